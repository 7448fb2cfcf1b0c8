// avirp.hip -- CImageResizer over single-channel PLANES (avirhip_resize_planes
// of include/avirhip.h with a CImageResizer plan of one channel): n planes of
// one geometry -- a channel-first image, a batch -- resized in ONE launch, both
// axes, with one float per lane.
//
// What such a plane costs on the plan's own road: it is zero-padded to float
// RGBA (four times the arithmetic) between a pack pass and an output stage, or,
// where no RGBA kernel takes the plan -- the filtered upsample the planner
// picks for small one-channel upsizing -- it runs one launch per op per axis.
// Here the source is read in the caller's element type and widened in the
// loader, every op of both axes runs on a tile in LDS, and the output stage is
// part of the store: no pack pass, no FltBuf, no scratch of the plan.
//
// k_avirp is a scalar LDS-tile interpreter of the plan's own lowered ops
// (plan.h: OP_FIR, OP_GATHER, OP_UPF behind VIEW_CLAMP / VIEW_ZS / VIEW_RAW),
// reading the plan's device tables. The defining text of the arithmetic is
// k_fir / k_gather / k_upf of generic.hip: every stored value receives the same
// products in the same order, sums start from +0.0f where they do there,
// multiply and add stay separate (-ffp-contract=off).
//
// Structure: a work item is (plane, tile of tw x tr outputs), the plane the
// slowest index, dealt round the 8 XCDs as k_lancp deals its items; a workgroup
// is AP_NT threads = 4 waves. Per tile the host has walked both chains
// backwards from the tile's outputs (ap_ranges: need_range's algebra, with an
// OP_UPF range of its own) and left, for every stage, the first stored index
// and the count the tile needs:
//   H chain, AP_RC source rows of [va0, va0 + vn0) at a time:
//     load  columns [ha0, ha0 + hn0) of the rows, widened
//     H ops stage s reads buffer s, writes buffer s + 1; the last one writes
//           the rows' tw results into F, which holds them for all vn0 rows
//   V ops on F's tw columns; the last one stores to global memory
// The buffers of a chain alternate between two LDS regions behind F, an
// s_barrier between stages: a decimating first filter (rf 4: 31 taps) reads a
// source tile of several hundred KB under 64 x 16 outputs, in row chunks it
// reads 32 rows of it at a time. A
// buffer of an OP_UPF holds SLOTS d = idx + out_prefix, which is what its
// consumer's VIEW_RAW addresses.
// Lanes run along image x in every stage. A V op's row of coefficients is
// wave-uniform (scalar loads). An H op's is per lane: a lane keeps AP_HQ rows
// in registers and loads each coefficient once for all of them.
// Row and plane addresses are formed in 64 bits.
//
// The tile is AP_TW x AP_TR unless its buffers exceed AP_LDS_PREF bytes: then
// the first of ap_cand that fits, else the first within AP_LDS_MAX.
//
// What avirp_run refuses (1; the caller runs the plan's road per plane) is
// listed in front of it.

#include "plan.h"
#include <algorithm>
#include <stdlib.h>
#include <stdio.h>

namespace avirhip {

#define AP_TW 64          // output columns per tile (first candidate)
#define AP_TR 16          // output rows per tile (first candidate)
#define AP_NT 256         // threads: 4 waves
#define AP_HQ 8           // rows a lane holds in an H op
#define AP_RC 32          // source rows the H chain runs at a time
#define AP_LDS_PREF 65536 // bytes of LDS a tile should stay within
#define AP_LDS_MAX 153600 // ... and may take
#define AP_MAXOPS 3       // ops per axis
// The largest plane the kernel keeps: max( source, result ) pixels of ONE plane
// (AVIRHIP_AVIRP_MAX_PIXELS, read per call, overrides it). The per-plane road
// costs 18-35 us a plane in launches whatever its size and very little per
// pixel (the RGBA kernels); k_avirp costs 0.02-0.04 us per 1000 pixels and no
// launches. Measured (NOTEBOOK 36, planar call against per-plane loop): 64 x 3
// planes 128x96 -> 256x192 0.30 / 6.82 ms, 64 x 3 planes 500x375 -> 224x224
// 0.89 / 4.57 ms; 3 planes 640x480 -> 1024x768 (786 432 pixels) 0.054 / 0.055:
// a tie; 3 planes 1920x1080 -> 2500x1400 0.222 / 0.153, 3840x2160 -> 1280x720
// 0.947 / 0.185, 1 plane 1920x1080 -> 3840x2160 0.162 / 0.051: behind.
#define AP_MAX_PIXELS 262144

// the tiles tried, in order (width, height)
static const int ap_cand[][ 2 ] = {{ AP_TW, AP_TR }, { 64, 8 }, { 32, 8 },
	{ 32, 4 }, { 16, 4 }};

enum { AP_U8 = 1, AP_U16 = 2, AP_F32 = 3, AP_F16 = 4, AP_BF16 = 5 };

template< int K > struct ApElem { typedef float T; };
template<> struct ApElem< AP_U8 > { typedef unsigned char T; };
template<> struct ApElem< AP_U16 > { typedef unsigned short T; };
template<> struct ApElem< AP_F16 > { typedef _Float16 T; };
template<> struct ApElem< AP_BF16 > { typedef __bf16 T; };

// one lowered op as the kernel reads it (pointers: the plan's device tables)
struct ApOp
{
	int type, view, in_len, in_prefix, zs_mmax;
	int rf, lat, e;
	int maxtaps;
	int flen, up_inprefix, up_R, sdc_len, pdc_len, pdc_d0;
	const float* flt;
	const int* start; const int* ntaps; const float* coef;
	const float* sdc; const float* pdc;
};

struct ApParams
{
	const char* src; long src_pb, src_sb; // row pitch, plane stride in bytes
	char* dst; long dst_pb, dst_sb;
	int nw, nh;
	int ntx, nty, tw, tr;
	int nhops, nvops;
	ApOp h[ AP_MAXOPS ], v[ AP_MAXOPS ];
	// per tile column / tile row: first stored index of buffers 0 .. nops
	// ([ 0 .. 3 ]) and their counts ([ 4 .. 7 ])
	const int* hr; const int* vr;
	int reg_a, reg_b; // first floats of the LDS regions A and B (F is at 0)
	int use_tr; float tr_mul, tr_muli, pk_out;
	// plane views (k_avirp< ., ., true >): plane i's source and result lie
	// where views[ i ] says; src, dst and the four pitches above are not read
	const PlaneViewDev* views;
};

// avir::round (avir.h:130-135) of the reference's x86-64 build, as generic.hip's
__device__ __forceinline__ float ap_round( const float d )
{
	return( d < 0.0f ? -(float) avirhip_x86_cvtt( 0.5f - d ) :
		(float) avirhip_x86_cvtt( d + 0.5f ));
}

// Output `o` of `op` for Q scanlines at once: element i of scanline q of the
// input buffer lies at in[ io[ q ] + ( i - in_a ) * is ] (H: io = row * pitch,
// is = 1; V: io = column, is = pitch). s[ q ] receives what k_fir / k_gather /
// k_upf store.
template< int Q >
__device__ __forceinline__ void ap_op( const ApOp& op, const int o,
	const float* const in, const int ( &io )[ Q ], const int is, const int in_a,
	float ( &s )[ Q ])
{
	// the view: logical index -> offset in the buffer; `z`: the element is a
	// zero of the zero-stuffed tail
	auto at = [&]( const int i, bool& z ) -> int
	{
		z = false;

		if( op.view == VIEW_RAW )
		{
			return(( i + op.in_prefix - in_a ) * is );
		}

		z = ( op.view == VIEW_ZS && i > op.zs_mmax );
		return(( min( max( i, 0 ), op.in_len - 1 ) - in_a ) * is );
	};

	if( op.type == OP_FIR )
	{
		const int cp = op.rf * ( o - op.e );
		bool z;
		const int a0 = at( cp, z );
		const float f0 = op.flt[ 0 ];
#pragma unroll
		for( int q = 0; q < Q; q++ )
		{
			s[ q ] = f0 * in[ io[ q ] + a0 ];
		}

		for( int i = 1; i <= op.lat; i++ )
		{
			const int ar = at( cp + i, z );
			const int al = at( cp - i, z );
			const float f = op.flt[ i ];
#pragma unroll
			for( int q = 0; q < Q; q++ )
			{
				s[ q ] += f * ( in[ io[ q ] + ar ] + in[ io[ q ] + al ]);
			}
		}
	}
	else
	if( op.type == OP_GATHER )
	{
		const int st = op.start[ o ];
		const int nt = op.ntaps[ o ];
		const float* const cf = op.coef + (long) o * op.maxtaps;
#pragma unroll
		for( int q = 0; q < Q; q++ )
		{
			s[ q ] = 0.0f;
		}

		for( int t = 0; t < nt; t++ )
		{
			bool z;
			const int a = at( st + t, z );
			const float f = cf[ t ];
#pragma unroll
			for( int q = 0; q < Q; q++ )
			{
				const float x = in[ io[ q ] + a ];
				s[ q ] += f * ( z ? 0.0f : x );
			}
		}
	}
	else
	{
		// (o is the slot d)
		int rlo = o - op.flen + 1;
		rlo = ( rlo <= 0 ? 0 : ( rlo + op.rf - 1 ) / op.rf );
		const int rhi = min( o / op.rf, op.up_R - 1 );
		const int ts = o - op.up_R * op.rf;
		const int tp = o - op.pdc_d0;
#pragma unroll
		for( int q = 0; q < Q; q++ )
		{
			s[ q ] = 0.0f;
		}

		for( int r = rlo; r <= rhi; r++ )
		{
			const int m = min( max( r - op.up_inprefix, 0 ), op.in_len - 1 );
			const int a = ( m - in_a ) * is;
			const float f = op.flt[ o - r * op.rf ];
#pragma unroll
			for( int q = 0; q < Q; q++ )
			{
				s[ q ] += f * in[ io[ q ] + a ];
			}
		}

		if( ts >= 0 && ts < op.sdc_len )
		{
			const int a = ( op.in_len - 1 - in_a ) * is;
			const float f = op.sdc[ ts ];
#pragma unroll
			for( int q = 0; q < Q; q++ )
			{
				s[ q ] += in[ io[ q ] + a ] * f;
			}
		}

		if( tp >= 0 && tp < op.pdc_len )
		{
			const int a = ( 0 - in_a ) * is;
			const float f = op.pdc[ tp ];
#pragma unroll
			for( int q = 0; q < Q; q++ )
			{
				s[ q ] += in[ io[ q ] + a ] * f;
			}
		}
	}
}

// VIEWS: as k_lancp's -- element (r, c) of a plane at base + r * pitch +
// c * estride bytes from the table P.views; loader and store alone differ, and
// the store stays a plain vector store of the element's own width.
template< int SRC, int OUT, bool VIEWS >
__global__ void __launch_bounds__( AP_NT ) k_avirp( const ApParams P )
{
	typedef typename ApElem< SRC > :: T src_t;
	typedef typename ApElem< OUT > :: T out_t;
	extern __shared__ __attribute__(( aligned( 16 ))) float ap_lds[];

	// (work items dealt round the 8 XCDs as k_lancp deals them)
	const int nwg = gridDim.x;
	const int b = blockIdx.x;
	const int xcd = b & 7;
	const int qd = nwg >> 3;
	const int rm = nwg & 7;
	const int item = ( xcd < rm ? xcd * ( qd + 1 ) :
		rm * ( qd + 1 ) + ( xcd - rm ) * qd ) + ( b >> 3 );

	const int per = P.ntx * P.nty;
	const int plane = item / per;
	const int tile = item - plane * per;
	const int ty = tile / P.ntx;
	const int tx = tile - ty * P.ntx;
	const int tid = threadIdx.x;
	const int wave = __builtin_amdgcn_readfirstlane( tid >> 6 );
	const int lane = tid & 63;
	const int tw = P.tw;

	const int* const hr = P.hr + tx * 8;
	const int* const vr = P.vr + ty * 8;
	int ha[ AP_MAXOPS + 1 ], hn[ AP_MAXOPS + 1 ];
	int va[ AP_MAXOPS + 1 ], vn[ AP_MAXOPS + 1 ];
#pragma unroll
	for( int i = 0; i <= AP_MAXOPS; i++ )
	{
		ha[ i ] = hr[ i ]; hn[ i ] = hr[ 4 + i ];
		va[ i ] = vr[ i ]; vn[ i ] = vr[ 4 + i ];
	}

	// (VIEWS: the plane's entry of the table; the dense form reads none of it)
	PlaneViewDev vw = PlaneViewDev();

	if constexpr( VIEWS )
	{
		vw = P.views[ plane ];
	}

	// LDS: F, the H chain's result for every source row of the tile (pitch
	// tw), and the two regions the stages alternate between
	const int rows = vn[ 0 ]; // source rows of the tile
	float* const F = ap_lds;
	float* const A = ap_lds + P.reg_a;
	float* const B = ap_lds + P.reg_b;

	// ---- the H chain, AP_RC source rows at a time: load (widened) -> A,
	// op i: buffer i -> buffer i + 1 (A, B, A ...), the last one into F
	for( int r0 = 0; r0 < rows; r0 += AP_RC )
	{
		const int nr = min( AP_RC, rows - r0 );
		float* cur = A;
		float* oth = B;

		{
			const char* const sp = ( VIEWS ? vw.src :
				P.src + (long) plane * P.src_sb ) + (long) ha[ 0 ] *
				( VIEWS ? vw.src_eb : (long) sizeof( src_t ));
			const int n = hn[ 0 ];

			for( int r = wave; r < nr; r += AP_NT / 64 )
			{
				const char* const row = sp +
					(long) ( va[ 0 ] + r0 + r ) *
					( VIEWS ? vw.src_pb : P.src_pb );

				for( int c = lane; c < n; c += 64 )
				{
					cur[ r * n + c ] = (float) pview_load< VIEWS, src_t >( row +
						(long) c *
						( VIEWS ? vw.src_eb : (long) sizeof( src_t )));
				}
			}
		}

		AVIRHIP_BARRIER_DRAIN();
		__syncthreads();
#pragma unroll
		for( int i = 0; i < AP_MAXOPS; i++ )
		{
			if( i < P.nhops )
			{
				const ApOp& op = P.h[ i ];
				const bool last = ( i == P.nhops - 1 );
				const int ip = hn[ i ];               // input pitch
				const int nval = hn[ i + 1 ];         // outputs that exist
				const int ncomp = ( last ? tw : nval ); // computed = pitch
				const int oa = ha[ i + 1 ];
				float* const out = ( last ? F + r0 * tw : oth );

				for( int c = lane; c < ncomp; c += 64 )
				{
					const int o = oa + min( c, nval - 1 );

					for( int rb = wave * AP_HQ; rb < nr;
						rb += ( AP_NT / 64 ) * AP_HQ )
					{
						int io[ AP_HQ ];
						float s[ AP_HQ ];
#pragma unroll
						for( int q = 0; q < AP_HQ; q++ )
						{
							io[ q ] = min( rb + q, nr - 1 ) * ip;
						}

						ap_op< AP_HQ >( op, o, cur, io, 1, ha[ i ], s );
#pragma unroll
						for( int q = 0; q < AP_HQ; q++ )
						{
							if( rb + q < nr )
							{
								out[ ( rb + q ) * ncomp + c ] = s[ q ];
							}
						}
					}
				}

				AVIRHIP_BARRIER_DRAIN();
				__syncthreads();
				float* const t = cur; cur = oth; oth = t;
			}
		}
	}

	// ---- V ops: on the tile's tw columns (pitch tw), the last one stores
	const int j = tx * tw + lane;
	const bool xok = ( lane < tw && j < P.nw );
	float* cur = F;
	float* oth = A;
#pragma unroll
	for( int i = 0; i < AP_MAXOPS; i++ )
	{
		if( i < P.nvops )
		{
			const ApOp& op = P.v[ i ];
			const bool last = ( i == P.nvops - 1 );
			const int nval = vn[ i + 1 ];
			const int oa = va[ i + 1 ];
			const int io[ 1 ] = { min( lane, tw - 1 )};

			for( int r = wave; r < nval; r += AP_NT / 64 )
			{
				float s[ 1 ];
				ap_op< 1 >( op, oa + r, cur, io, tw, va[ i ], s );

				if( !last )
				{
					if( lane < tw )
					{
						oth[ r * tw + lane ] = s[ 0 ];
					}

					continue;
				}

				if( !xok )
				{
					continue;
				}

				// the output stage (k_epilogue_px of generic.hip) in the store
				float t = s[ 0 ];
				char* const dp =
					( VIEWS ? vw.dst : P.dst + (long) plane * P.dst_sb ) +
					(long) ( oa + r ) * ( VIEWS ? vw.dst_pb : P.dst_pb ) +
					(long) j * ( VIEWS ? vw.dst_eb : (long) sizeof( out_t ));

				if constexpr( OUT == AP_U8 || OUT == AP_U16 )
				{
					t = ( P.use_tr ? ap_round( t * P.tr_muli ) * P.tr_mul :
						ap_round( t ));
					t = ( t < 0.0f ? 0.0f : ( t > P.pk_out ? P.pk_out : t ));
				}

				// (half: v_cvt_f16_f32, bfloat16: the compiler's conversion --
				// both nearest even, denormals kept; float as it is)
				pview_store< VIEWS, out_t >( dp, (out_t) t );
			}

			if( !last )
			{
				AVIRHIP_BARRIER_DRAIN();
				__syncthreads();
				cur = oth;
				oth = ( cur == A ? B : A );
			}
		}
	}
}

// ---------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------

namespace {

// The stored indices [*ia, *ib] of its input buffer that `op` reads for the
// stored indices [a, b] of its output buffer (slots for an OP_UPF, logical
// indices otherwise). need_range's algebra (api.cpp) with an OP_UPF range of its
// own: the inputs of [rlo( a ), rhi( b )] - up_inprefix, widened to the last /
// first input sample where the slots reach the SuffixDC / PrefixDC ranges.
bool ap_need( const LOp& op, const int a, const int b, int* ia, int* ib )
{
	if( op.type != OP_UPF )
	{
		need_range( op, a, b, *ia, *ib );

		if( op.view == VIEW_RAW )
		{
			*ia += op.in_prefix;
			*ib += op.in_prefix;
		}

		return( *ia <= *ib );
	}

	if( a < 0 || b >= op.out_total )
	{
		return( false );
	}

	int lo = 0x7fffffff, hi = -0x7fffffff;
	int rlo = a - op.flen + 1;
	rlo = ( rlo <= 0 ? 0 : ( rlo + op.rf - 1 ) / op.rf );
	const int rhi = std::min( b / op.rf, op.up_R - 1 );

	if( rlo <= rhi )
	{
		lo = std::max( 0, std::min( rlo - op.up_inprefix, op.in_len - 1 ));
		hi = std::max( 0, std::min( rhi - op.up_inprefix, op.in_len - 1 ));
	}

	if( op.sdc_len > 0 && b >= op.up_R * op.rf &&
		a < op.up_R * op.rf + op.sdc_len )
	{
		lo = std::min( lo, op.in_len - 1 );
		hi = std::max( hi, op.in_len - 1 );
	}

	if( op.pdc_len > 0 && b >= op.pdc_d0 && a < op.pdc_d0 + op.pdc_len )
	{
		lo = std::min( lo, 0 );
		hi = std::max( hi, 0 );
	}

	if( lo > hi )
	{
		// slots nothing contributes to (+0.0f): any sample will do
		lo = 0; hi = 0;
	}

	*ia = lo; *ib = hi;
	return( true );
}

// the table of one axis for tiles of `t` outputs: 8 ints per tile (ApParams)
bool ap_ranges( const LAxis& ax, const int t, std::vector< int >& tab,
	int ( &maxn )[ AP_MAXOPS + 1 ])
{
	const int n = (int) ax.ops.size();
	const int nt = ( ax.dst_len + t - 1 ) / t;
	tab.assign( (size_t) nt * 8, 0 );

	for( int i = 0; i <= AP_MAXOPS; i++ )
	{
		maxn[ i ] = 0;
	}

	for( int k = 0; k < nt; k++ )
	{
		int a = k * t, b = std::min( a + t, ax.dst_len ) - 1;
		int* const r = &tab[ (size_t) k * 8 ];
		r[ n ] = a; r[ 4 + n ] = b - a + 1;

		for( int i = n - 1; i >= 0; i-- )
		{
			const LOp& op = ax.ops[ i ];

			// (the buffer a VIEW_RAW op reads is the OP_UPF's in front of it)
			if(( op.view == VIEW_RAW ) !=
				( i > 0 && ax.ops[ i - 1 ].type == OP_UPF ) ||
				( op.view == VIEW_RAW &&
				op.in_prefix != ax.ops[ i - 1 ].out_prefix ))
			{
				return( false );
			}

			int ia, ib;

			if( !ap_need( op, a, b, &ia, &ib ))
			{
				return( false );
			}

			a = ia; b = ib;
			r[ i ] = a; r[ 4 + i ] = b - a + 1;
		}

		if( a < 0 || b >= ax.src_len )
		{
			return( false );
		}

		for( int i = 0; i <= n; i++ )
		{
			maxn[ i ] = std::max( maxn[ i ], r[ 4 + i ]);
		}
	}

	return( true );
}

// The planar state of a plan: made on the first planar call, under the plan's
// mutex; read without a lock afterwards (avirhip_plan::avirp).
struct AvirpData
{
	int ok;           // 0: refused, for `why`
	const char* why;
	int tw, tr, ntx, nty;
	int reg_a, reg_b, lds; // floats in front of regions A, B; bytes of all
	int* d_hr; int* d_vr;
};

// floats of the LDS regions a tile takes: F, the H chain's result (the tile's
// source rows x tw); A and B, which hold the H chain's buffers 0 .. nh - 1 for
// AP_RC rows (buffer s in region s & 1) and then the V chain's buffers
// 1 .. nv - 1 (rows x tw; buffer i in region ( i - 1 ) & 1)
void ap_lds_of( const int nh, const int nv, const int tw,
	const int ( &hm )[ AP_MAXOPS + 1 ], const int ( &vm )[ AP_MAXOPS + 1 ],
	long ( &reg )[ 3 ])
{
	reg[ 0 ] = 0; reg[ 1 ] = 0;
	reg[ 2 ] = (long) vm[ 0 ] * tw;
	const long rc = std::min( vm[ 0 ], AP_RC );

	for( int s = 0; s < nh; s++ )
	{
		reg[ s & 1 ] = std::max( reg[ s & 1 ], rc * hm[ s ]);
	}

	for( int i = 1; i < nv; i++ )
	{
		reg[ ( i - 1 ) & 1 ] = std::max( reg[ ( i - 1 ) & 1 ],
			(long) vm[ i ] * tw );
	}
}

AvirpData* ap_make( avirhip_plan* p )
{
	AvirpData* const D = new AvirpData();
	D -> ok = 0; D -> why = ""; D -> d_hr = nullptr; D -> d_vr = nullptr;
	const int nh = (int) p -> h.ops.size();
	const int nv = (int) p -> v.ops.size();

	if( nh < 1 || nv < 1 || nh > AP_MAXOPS || nv > AP_MAXOPS )
	{
		D -> why = "chain of more than three ops";
		return( D );
	}

	std::vector< int > hr, vr, bhr, bvr;
	int best = -1;
	long best_lds = 0, best_a = 0, best_b = 0;
	D -> why = "tile exceeds LDS";

	for( int c = 0; c < (int) ( sizeof( ap_cand ) / sizeof( ap_cand[ 0 ])); c++ )
	{
		int hm[ AP_MAXOPS + 1 ], vm[ AP_MAXOPS + 1 ];

		if( !ap_ranges( p -> h, ap_cand[ c ][ 0 ], hr, hm ) ||
			!ap_ranges( p -> v, ap_cand[ c ][ 1 ], vr, vm ))
		{
			D -> why = "op ranges";
			return( D );
		}

		long reg[ 3 ];
		ap_lds_of( nh, nv, ap_cand[ c ][ 0 ], hm, vm, reg );
		const long lds = ( reg[ 0 ] + reg[ 1 ] + reg[ 2 ]) *
			(long) sizeof( float );

		if( lds <= AP_LDS_PREF || ( best < 0 && lds <= AP_LDS_MAX ))
		{
			best = c; best_lds = lds; best_a = reg[ 2 ];
			best_b = reg[ 2 ] + reg[ 0 ];
			bhr = hr; bvr = vr;

			if( lds <= AP_LDS_PREF )
			{
				break;
			}
		}
	}

	if( best < 0 )
	{
		return( D );
	}

	D -> tw = ap_cand[ best ][ 0 ]; D -> tr = ap_cand[ best ][ 1 ];
	D -> ntx = ( p -> new_w + D -> tw - 1 ) / D -> tw;
	D -> nty = ( p -> new_h + D -> tr - 1 ) / D -> tr;
	D -> reg_a = (int) best_a; D -> reg_b = (int) best_b;
	D -> lds = (int) best_lds;

	if( hipMalloc( (void**) &D -> d_hr, bhr.size() * sizeof( int )) !=
		hipSuccess || hipMalloc( (void**) &D -> d_vr, bvr.size() *
		sizeof( int )) != hipSuccess ||
		hipMemcpy( D -> d_hr, bhr.data(), bhr.size() * sizeof( int ),
		hipMemcpyHostToDevice ) != hipSuccess ||
		hipMemcpy( D -> d_vr, bvr.data(), bvr.size() * sizeof( int ),
		hipMemcpyHostToDevice ) != hipSuccess )
	{
		(void) hipGetLastError();
		D -> why = "range tables";
		return( D );
	}

	D -> why = "";
	D -> ok = 1;
	return( D );
}

void ap_fill_op( const LOp& s, ApOp& d )
{
	d.type = s.type; d.view = s.view; d.in_len = s.in_len;
	d.in_prefix = s.in_prefix; d.zs_mmax = s.zs_mmax;
	d.rf = s.rf; d.lat = s.lat; d.e = s.e; d.maxtaps = s.maxtaps;
	d.flen = s.flen; d.up_inprefix = s.up_inprefix; d.up_R = s.up_R;
	d.sdc_len = s.sdc_len; d.pdc_len = s.pdc_len; d.pdc_d0 = s.pdc_d0;
	d.flt = s.d_flt; d.start = s.d_start; d.ntaps = s.d_ntaps;
	d.coef = s.d_coef; d.sdc = s.d_sdc; d.pdc = s.d_pdc;
}

template< int SK >
void ap_launch( const int ok, const long items, const size_t lds,
	hipStream_t st, const ApParams& P, hipError_t* e )
{
#define AP_GO1( OK, VW ) { *e = AVIRHIP_DYN_LDS(( k_avirp< SK, OK, VW > ), lds ); \
		if( *e == hipSuccess ) hipLaunchKernelGGL(( k_avirp< SK, OK, VW > ), \
		dim3( (unsigned) items ), dim3( AP_NT ), lds, st, P ); }
#define AP_GO( OK ) { if( P.views != nullptr ) AP_GO1( OK, true ) \
		else AP_GO1( OK, false ) }

	switch( ok )
	{
		case AP_U8: AP_GO( AP_U8 ); break;
		case AP_U16: AP_GO( AP_U16 ); break;
		case AP_F16: AP_GO( AP_F16 ); break;
		case AP_BF16: AP_GO( AP_BF16 ); break;
		default: AP_GO( AP_F32 ); break;
	}
#undef AP_GO
#undef AP_GO1
}

} // namespace

void avirp_release( avirhip_plan* p )
{
	AvirpData* const D = (AvirpData*) p -> avirp.load();

	if( D != nullptr )
	{
		if( D -> d_hr != nullptr ) (void) hipFree( D -> d_hr );
		if( D -> d_vr != nullptr ) (void) hipFree( D -> d_vr );
		delete D;
		p -> avirp.store( nullptr );
	}
}

// The planes of `p` (a CImageResizer plan of one channel): `n_planes` source
// planes `src_ps` elements apart behind `src`, their results `dst_ps` elements
// apart behind `dst`, rows at the plan's pitches -- or, with `views`, each
// plane where its entry of that host table says (validated by the caller);
// device memory, asynchronous on `st`. 1: the call is not this kernel's, nothing was launched and `*why`
// says what it missed:
//   element type        float64 on a side: no loader / store for it
//   plan stages         sRGB gamma, the error-diffusion ditherer, fpclass_float4,
//                       fpclass_def<double>: stages the kernel does not have
//   base alignment      a base that is no multiple of the element size
//   chain of more than three ops (none found so far); op ranges (a chain
//                       whose views are not the lowering's)
//   tile exceeds LDS    no candidate tile within AP_LDS_MAX
//   work items          more than 2^31 - 1
//   plane above AVIRHIP_AVIRP_MAX_PIXELS: a plane of more than AP_MAX_PIXELS
//                       source or result pixels, where the per-plane road
//                       measured level or faster (see AP_MAX_PIXELS)
//   AVIRHIP_AVIRP_OFF   set in the environment (read per call): the
//                       measurement's switch for the per-plane road
int avirp_run( avirhip_plan* p, const void* src, void* dst, long src_ps,
	long dst_ps, int n_planes, hipStream_t st, const char** why,
	const PlaneViewTable* views )
{
	const int sk = gp_raw_kind( p -> in_type );
	const int ok = gp_raw_kind( p -> out_type );

	if( sk == 0 || ok == 0 )
	{
		*why = "element type";
		return( 1 );
	}

	if( p -> gamma || p -> f64 || p -> fp4 ||
		p -> dither != AVIRHIP_DITHER_DEF )
	{
		*why = "plan stages";
		return( 1 );
	}

	if( views == nullptr &&
		( (uintptr_t) src % dtype_size( p -> in_type ) != 0 ||
		(uintptr_t) dst % dtype_size( p -> out_type ) != 0 ))
	{
		*why = "base alignment";
		return( 1 );
	}

	if( getenv( "AVIRHIP_AVIRP_OFF" ) != nullptr )
	{
		*why = "AVIRHIP_AVIRP_OFF";
		return( 1 );
	}

	{
		const char* const e = getenv( "AVIRHIP_AVIRP_MAX_PIXELS" );
		const long long cap = ( e != nullptr ? atoll( e ) : AP_MAX_PIXELS );

		if( std::max( (long long) p -> src_w * p -> src_h,
			(long long) p -> new_w * p -> new_h ) > cap )
		{
			*why = "plane above AVIRHIP_AVIRP_MAX_PIXELS";
			return( 1 );
		}
	}

	AvirpData* D = (AvirpData*) p -> avirp.load( std::memory_order_acquire );

	if( D == nullptr )
	{
		std::lock_guard< std::mutex > lock( p -> avirp_mtx );
		D = (AvirpData*) p -> avirp.load( std::memory_order_acquire );

		if( D == nullptr )
		{
			D = ap_make( p );
			p -> avirp.store( D, std::memory_order_release );
		}
	}

	if( !D -> ok )
	{
		*why = D -> why;
		return( 1 );
	}

	const long items = (long) D -> ntx * D -> nty * n_planes;

	if( items > 0x7fffffffL )
	{
		*why = "work items";
		return( 1 );
	}

	ApParams P;
	const long ses = (long) dtype_size( p -> in_type );
	const long oes = (long) dtype_size( p -> out_type );
	P.src = (const char*) src;
	P.src_pb = (long) p -> src_stride * ses; P.src_sb = src_ps * ses;
	P.dst = (char*) dst;
	P.dst_pb = (long) p -> new_stride * oes; P.dst_sb = dst_ps * oes;
	P.nw = p -> new_w; P.nh = p -> new_h;
	P.ntx = D -> ntx; P.nty = D -> nty; P.tw = D -> tw; P.tr = D -> tr;
	P.nhops = (int) p -> h.ops.size(); P.nvops = (int) p -> v.ops.size();

	for( int i = 0; i < AP_MAXOPS; i++ )
	{
		ap_fill_op( p -> h.ops[ std::min( i, P.nhops - 1 )], P.h[ i ]);
		ap_fill_op( p -> v.ops[ std::min( i, P.nvops - 1 )], P.v[ i ]);
	}

	P.hr = D -> d_hr; P.vr = D -> d_vr;
	P.reg_a = D -> reg_a; P.reg_b = D -> reg_b;
	P.use_tr = ( p -> tr_mul != 1.0 );
	P.tr_mul = (float) p -> tr_mul;
	P.tr_muli = (float) ( 1.0 / p -> tr_mul );
	P.pk_out = (float) p -> pk_out;
	P.views = nullptr;
	PlaneViewUpload up;

	if( views != nullptr )
	{
		// (the last refusal is behind us: the table travels only to a launch)
		const int rc = up.push( *views, p -> device, st );

		if( rc != 0 )
		{
			return( rc );
		}

		P.views = up.dev();
	}

	if( getenv( "AVIRHIP_VERBOSE" ) != nullptr )
	{
		fprintf( stderr, "k_avirp: %ld items (planes %d, tile %dx%d, ops %d+%d, "
			"lds %d)\n", items, n_planes, D -> tw, D -> tr, P.nhops, P.nvops,
			D -> lds );
	}

	const size_t lds = (size_t) D -> lds;
	hipError_t e = hipSuccess;

	switch( sk )
	{
		case AP_U8: ap_launch< AP_U8 >( ok, items, lds, st, P, &e ); break;
		case AP_U16: ap_launch< AP_U16 >( ok, items, lds, st, P, &e ); break;
		case AP_F16: ap_launch< AP_F16 >( ok, items, lds, st, P, &e ); break;
		case AP_BF16: ap_launch< AP_BF16 >( ok, items, lds, st, P, &e ); break;
		default: ap_launch< AP_F32 >( ok, items, lds, st, P, &e ); break;
	}

	up.done( st );
	AVIRHIP_HIPCHECK( e );
	AVIRHIP_HIPCHECK( hipGetLastError() );
	return( AVIRHIP_OK );
}

} // namespace avirhip
