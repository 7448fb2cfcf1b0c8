// lancp.hip -- LANCIR over single-channel PLANES (avirhip_resize_planes of
// include/avirhip.h): n planes of one geometry -- a channel-first image, a
// batch -- resized in ONE launch, both passes, with one float per lane.
//
// The arithmetic is the reference's 1-channel image (resize1, lancir.h:2102-),
// as lancir_dot< 1 > of generic.hip spells it out, bit for bit: vertical pass
// first, indices clamped to the frame, no contraction, and on both axes four
// lane sums over the taps 4g + L whose first terms are bare products,
//   ( s0 + s2 ) + ( s1 + s3 ),
// a kernel length with kl % 4 == 2 adding its last two taps to the two partial
// sums first. Behind it the gain ( v * out_mul unless the plan is unity ) and
// the output stage by the element's position in its scanline of new_w
// elements (k_lancir_out of generic.hip): integer elements clamp, whole groups
// of four round to nearest even, the 1-3 element tail by + 0.5 truncation; half
// and bfloat16 narrow to nearest even with no clamp; float is stored as it is.
//
// What every other CLancIR kernel of this library does for such an image is
// compute it zero-padded to float RGBA in an inner plan, between a pack pass
// and an output stage: four times the arithmetic and two float copies of the
// frame per plane. Here the source is read in the caller's element type and
// widened in the loader, and the result is converted in the store.
//
// Structure: a work item is (plane, tile of LP_TW output columns x LP_TR
// output rows), dealt round the 8 XCDs as k_lanc2h deals them with the plane
// as the slowest index; a workgroup is LP_NT threads = 4 waves.
//   V  for the tile's output rows and the source columns [cx0, cx1] its
//      horizontal taps read (clamped to the frame): a wave takes one output row
//      at a time (rows wave, wave + 4, ...: the row's filter is uniform, scalar
//      loads), its lanes run along x -- coalesced loads in the caller's element
//      type. The intermediate rows go to LDS as floats.
//   barrier
//   H  a lane is one output column (tid & 63) and LP_TR / 4 output rows (wave,
//      wave + 4, ...): the taps of its own phase ( d_fidx[ j ] ) are loaded
//      once per group of four and used for all of its rows. Its position, its
//      phase and its first four taps are loaded before the V pass.
// LDS banks: column x of an intermediate row lies at float x + ( x >> 5 ) of
// it -- one float of padding behind every 32. ds_read_b32 is served in two
// groups of 32 lanes over 32 banks; a downsizing H pass reads with a stride of
// about k floats between lanes, and with the skew the strides 2, 4, 8 and 16
// touch 32 different banks (without it: 2, 4, 8, 16 lanes per bank). Upsizing
// reads neighbouring or equal addresses (conflict-free / broadcast), the V
// pass stores consecutive ones.
// Row and plane addresses are formed in 64 bits
// ( base + (long) plane * stride + (long) row * pitch ): no distance limit
// exists and the host checks none. With plane views (AVIRHIP_MEM_VIEWS) a
// plane's base, row pitch and element stride come from a table instead, by
// plane: the VIEWS instantiation below, whose loader and store alone differ.
//
// The kernel allocates nothing and uses no scratch of the plan: calls on one
// plan need no lock.
//
// What lancp_run refuses (1; the caller runs the plan's own road per plane):
// an element type outside uint8, uint16, float, half, bfloat16; a base that is
// no multiple of the element size; a geometry whose tile of intermediate rows
// exceeds LP_LDS bytes (very long kernels: KernelLen = 2 ceil( la max( 1, k )),
// lancir.h:893-895).

#include "plan.h"
#include <algorithm>

namespace avirhip {

#define LP_TW 64        // output columns per tile
// (32 rows: as fast when upsizing, 1.4x SLOWER at 3840x2160 -> 1280x720, whose
// 27 KB tiles leave a CU five workgroups -- NOTEBOOK 35)
#define LP_TR 16        // output rows per tile
#define LP_NT 256       // threads: 4 waves
#define LP_LDS 65536    // bytes of LDS a tile's intermediate rows may take

// element kinds of the kernel's two sides: gp_raw_kind's (plan.h)
enum { LP_U8 = 1, LP_U16 = 2, LP_F32 = 3, LP_F16 = 4, LP_BF16 = 5 };

template< int K > struct LpElem { typedef float T; };
template<> struct LpElem< LP_U8 > { typedef unsigned char T; };
template<> struct LpElem< LP_U16 > { typedef unsigned short T; };
template<> struct LpElem< LP_F16 > { typedef _Float16 T; };
template<> struct LpElem< LP_BF16 > { typedef __bf16 T; };

struct LancpParams
{
	const char* src; long src_pb, src_sb; // row pitch, plane stride in bytes
	char* dst; long dst_pb, dst_sb;
	int sw, sh, nw, nh;
	int ntx, nty;  // tiles along x, along y (per plane)
	int pitch;     // floats per intermediate row in LDS
	const int* vstart; const int* vfidx; const float* vflt; int vkl;
	const int* hstart; const int* hfidx; const float* hflt; int hkl;
	int unity; float out_mul, clampv;
	int l4;        // new_w & ~3: the elements that round to nearest even
	// plane views (k_lancp< ., ., true >): plane i's source and result lie
	// where views[ i ] says; src, dst and the four pitches above are not read
	const PlaneViewDev* views;
};

// position of column x in an intermediate row (see "LDS banks" above)
__device__ __forceinline__ int lp_skew( const int x )
{
	return( x + ( x >> 5 ));
}

// VIEWS: element (r, c) of a plane lies at base + r * pitch + c * estride
// bytes, the three read from the table P.views by plane (one load of 48 bytes
// per workgroup, uniform: scalar). Everything between the loader and the
// store is the dense form's. The store stays a plain vector store of the
// element's own width: interleaved result planes are written by other
// workgroups, on other XCDs, into the same cache lines, whose L2s keep dirty
// bytes apart -- a store widened to its neighbours would write them back stale.
template< int SRC, int OUT, bool VIEWS >
__global__ void __launch_bounds__( LP_NT ) k_lancp( const LancpParams P )
{
	typedef typename LpElem< SRC > :: T src_t;
	typedef typename LpElem< OUT > :: T out_t;
	extern __shared__ __attribute__(( aligned( 16 ))) float lp_sT[];
	float* const sT = lp_sT; // [LP_TR][P.pitch]

	// (work items dealt round the 8 XCDs as k_lanc2h deals them)
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

	const int j0 = tx * LP_TW;
	const int j1 = min( j0 + LP_TW, P.nw );
	const int y0 = ty * LP_TR;
	const int vkl = P.vkl, hkl = P.hkl;

	// the source columns this tile's horizontal taps read (d_start does not
	// decrease along the axis: lancp_run checks)
	const int cx0 = min( max( P.hstart[ j0 ], 0 ), P.sw - 1 );
	const int cx1 = min( max( P.hstart[ j1 - 1 ] + hkl - 1, 0 ), P.sw - 1 );
	const int S = cx1 - cx0 + 1;

	// (VIEWS: the plane's entry of the table; the dense form reads none of it)
	PlaneViewDev vw = PlaneViewDev();

	if constexpr( VIEWS )
	{
		vw = P.views[ plane ];
	}

	const char* const splane = ( VIEWS ? vw.src :
		P.src + (long) plane * P.src_sb );

	// the H pass' own position and phase: loaded here, so that they travel
	// while the V pass runs
	constexpr int NR = LP_TR / ( LP_NT / 64 ); // rows per wave and per lane
	const int j = j0 + lane;
	const bool xok = ( j < P.nw );
	const int jc = min( j, P.nw - 1 );
	const int hs = P.hstart[ jc ];
	const float* const hf = P.hflt + (long) P.hfidx[ jc ] * hkl;
	const float hf0 = hf[ 0 ], hf1 = hf[ 1 ], hf2 = hf[ 2 ], hf3 = hf[ 3 ];

	// ---- V: source rows -> the tile's intermediate rows
	// (the rows' positions and filters up front: independent scalar loads)
	int vst[ NR ], vfi[ NR ];
#pragma unroll
	for( int i = 0; i < NR; i++ )
	{
		const int y = min( y0 + wave + i * ( LP_NT / 64 ), P.nh - 1 );
		vst[ i ] = P.vstart[ y ];
		vfi[ i ] = P.vfidx[ y ];
	}

#pragma unroll
	for( int i = 0; i < NR; i++ )
	{
		const int r = wave + i * ( LP_NT / 64 );

		if( y0 + r >= P.nh )
		{
			break;
		}

		const int st = vst[ i ];
		const float* const f = P.vflt + (long) vfi[ i ] * vkl;
		float* const trow = sT + r * P.pitch;

		for( int c = lane; c < S; c += 64 )
		{
			const char* const col = splane + (long) ( cx0 + c ) *
				( VIEWS ? vw.src_eb : (long) sizeof( src_t ));

			auto px = [&]( const int t ) -> float
			{
				const int yy = min( max( st + t, 0 ), P.sh - 1 );
				return( (float) pview_load< VIEWS, src_t >( col + (long) yy *
					( VIEWS ? vw.src_pb : P.src_pb )));
			};

			float s0 = f[ 0 ] * px( 0 ), s1 = f[ 1 ] * px( 1 );
			float s2 = f[ 2 ] * px( 2 ), s3 = f[ 3 ] * px( 3 );

			for( int q = 4; q + 3 < vkl; q += 4 )
			{
				s0 += f[ q ] * px( q );
				s1 += f[ q + 1 ] * px( q + 1 );
				s2 += f[ q + 2 ] * px( q + 2 );
				s3 += f[ q + 3 ] * px( q + 3 );
			}

			float v;

			if(( vkl & 3 ) == 0 )
			{
				v = ( s0 + s2 ) + ( s1 + s3 );
			}
			else
			{
				const float e0 = f[ vkl - 2 ] * px( vkl - 2 );
				const float e1 = f[ vkl - 1 ] * px( vkl - 1 );
				v = (( s0 + s2 ) + e0 ) + (( s1 + s3 ) + e1 );
			}

			trow[ lp_skew( c )] = v;
		}
	}

	AVIRHIP_BARRIER_DRAIN();
	__syncthreads();

	// ---- H: the intermediate rows -> the tile's output rows
	const float* const tb = sT + wave * P.pitch;
	const int rstep = ( LP_NT / 64 ) * P.pitch;

	auto at = [&]( const int t ) -> int
	{
		return( lp_skew( min( max( hs + t, 0 ), P.sw - 1 ) - cx0 ));
	};

	float s[ NR ][ 4 ];

	{
		const int a0 = at( 0 ), a1 = at( 1 ), a2 = at( 2 ), a3 = at( 3 );
		const float f0 = hf0, f1 = hf1, f2 = hf2, f3 = hf3;
#pragma unroll
		for( int i = 0; i < NR; i++ )
		{
			const float* const t = tb + i * rstep;
			s[ i ][ 0 ] = f0 * t[ a0 ];
			s[ i ][ 1 ] = f1 * t[ a1 ];
			s[ i ][ 2 ] = f2 * t[ a2 ];
			s[ i ][ 3 ] = f3 * t[ a3 ];
		}
	}

	for( int q = 4; q + 3 < hkl; q += 4 )
	{
		const int a0 = at( q ), a1 = at( q + 1 ), a2 = at( q + 2 );
		const int a3 = at( q + 3 );
		const float f0 = hf[ q ], f1 = hf[ q + 1 ], f2 = hf[ q + 2 ];
		const float f3 = hf[ q + 3 ];
#pragma unroll
		for( int i = 0; i < NR; i++ )
		{
			const float* const t = tb + i * rstep;
			s[ i ][ 0 ] += f0 * t[ a0 ];
			s[ i ][ 1 ] += f1 * t[ a1 ];
			s[ i ][ 2 ] += f2 * t[ a2 ];
			s[ i ][ 3 ] += f3 * t[ a3 ];
		}
	}

	float o[ NR ];

	if(( hkl & 3 ) == 0 )
	{
#pragma unroll
		for( int i = 0; i < NR; i++ )
		{
			o[ i ] = ( s[ i ][ 0 ] + s[ i ][ 2 ]) + ( s[ i ][ 1 ] + s[ i ][ 3 ]);
		}
	}
	else
	{
		const int a0 = at( hkl - 2 ), a1 = at( hkl - 1 );
		const float f0 = hf[ hkl - 2 ], f1 = hf[ hkl - 1 ];
#pragma unroll
		for( int i = 0; i < NR; i++ )
		{
			const float* const t = tb + i * rstep;
			const float e0 = f0 * t[ a0 ];
			const float e1 = f1 * t[ a1 ];
			o[ i ] = (( s[ i ][ 0 ] + s[ i ][ 2 ]) + e0 ) +
				(( s[ i ][ 1 ] + s[ i ][ 3 ]) + e1 );
		}
	}

	// ---- gain, output stage by position, store
	char* const dcol = ( VIEWS ? vw.dst : P.dst + (long) plane * P.dst_sb ) +
		(long) j * ( VIEWS ? vw.dst_eb : (long) sizeof( out_t ));
#pragma unroll
	for( int i = 0; i < NR; i++ )
	{
		const int y = y0 + wave + i * ( LP_NT / 64 );

		if( !xok || y >= P.nh )
		{
			continue;
		}

		float v = o[ i ];

		if( !P.unity )
		{
			v = v * P.out_mul;
		}

		char* const op = dcol + (long) y * ( VIEWS ? vw.dst_pb : P.dst_pb );

		if constexpr( OUT == LP_U8 || OUT == LP_U16 )
		{
			if( j < P.l4 )
			{
				v = ( v < P.clampv ? v : P.clampv );
				v = ( v > 0.0f ? v : 0.0f );
				pview_store< VIEWS, out_t >( op, (out_t) (int) rintf( v ));
			}
			else
			{
				pview_store< VIEWS, out_t >( op, (out_t) (int) (( v > P.clampv ?
					P.clampv : ( v < 0.0f ? 0.0f : v )) + 0.5f ));
			}
		}
		else
		{
			// (float as it is; half: v_cvt_f16_f32, bfloat16: the compiler's
			// conversion -- both nearest even, as k_lancir_out's (Tout) v)
			pview_store< VIEWS, out_t >( op, (out_t) v );
		}
	}
}

// ---------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------

// The planes of `p` (a CLancIR plan of one channel): `n_planes` source planes
// `src_ps` elements apart behind `src`, their results `dst_ps` elements apart
// behind `dst`, rows at the plan's pitches -- or, with `views`, each plane
// where its entry of that host table says (src, dst and the strides are not
// used; the caller has validated the table); device memory, asynchronous on
// `st`. 1: the call is not this kernel's, nothing was launched and `*why`
// says what it missed.
int lancp_run( const avirhip_plan* p, const void* src, void* dst, long src_ps,
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

	if( views == nullptr &&
		( (uintptr_t) src % dtype_size( p -> in_type ) != 0 ||
		(uintptr_t) dst % dtype_size( p -> out_type ) != 0 ))
	{
		*why = "base alignment";
		return( 1 );
	}

	const LancirAxisDev& V = p -> lv;
	const LancirAxisDev& H = p -> lh;

	if( V.kernel_len < 4 || H.kernel_len < 4 || ( V.kernel_len & 1 ) != 0 ||
		( H.kernel_len & 1 ) != 0 || (int) H.h_start.size() != p -> new_w ||
		(int) V.h_start.size() != p -> new_h )
	{
		*why = "kernel length";
		return( 1 );
	}

	// the widest span of source columns a tile's taps read, as the kernel
	// forms it; d_start must not decrease (the tile's first and last column
	// bound every lane's reads)
	const int ntx = ( p -> new_w + LP_TW - 1 ) / LP_TW;
	const int nty = ( p -> new_h + LP_TR - 1 ) / LP_TR;
	int span = 1;

	for( int j = 1; j < p -> new_w; j++ )
	{
		if( H.h_start[ j ] < H.h_start[ j - 1 ])
		{
			*why = "tap positions";
			return( 1 );
		}
	}

	for( int tx = 0; tx < ntx; tx++ )
	{
		const int j0 = tx * LP_TW;
		const int j1 = std::min( j0 + LP_TW, p -> new_w );
		const int cx0 = std::min( std::max( H.h_start[ j0 ], 0 ),
			p -> src_w - 1 );
		const int cx1 = std::min( std::max( H.h_start[ j1 - 1 ] +
			H.kernel_len - 1, 0 ), p -> src_w - 1 );
		span = std::max( span, cx1 - cx0 + 1 );
	}

	const int pitch = span + ( span >> 5 ) + 1;
	const size_t lds = (size_t) LP_TR * pitch * sizeof( float );

	if( lds > LP_LDS )
	{
		*why = "tile exceeds LDS";
		return( 1 );
	}

	const long items = (long) ntx * nty * n_planes;

	if( items > 0x7fffffffL )
	{
		*why = "work items";
		return( 1 );
	}

	LancpParams P;
	const long ses = (long) dtype_size( p -> in_type );
	const long oes = (long) dtype_size( p -> out_type );
	P.src = (const char*) src;
	P.src_pb = (long) p -> src_stride * ses; P.src_sb = src_ps * ses;
	P.dst = (char*) dst;
	P.dst_pb = (long) p -> new_stride * oes; P.dst_sb = dst_ps * oes;
	P.sw = p -> src_w; P.sh = p -> src_h;
	P.nw = p -> new_w; P.nh = p -> new_h;
	P.ntx = ntx; P.nty = nty; P.pitch = pitch;
	P.vstart = V.d_start; P.vfidx = V.d_fidx; P.vflt = V.d_flt;
	P.vkl = V.kernel_len;
	P.hstart = H.d_start; P.hfidx = H.d_fidx; P.hflt = H.d_flt;
	P.hkl = H.kernel_len;
	P.unity = p -> l_unity; P.out_mul = p -> l_out_mul;
	P.clampv = p -> l_clamp;
	P.l4 = p -> new_w & ~3;
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
		fprintf( stderr, "k_lancp: %ld items (planes %d, tile %dx%d, span %d, "
			"lds %d)\n", items, n_planes, LP_TW, LP_TR, span, (int) lds );
	}

#define LP_LAUNCH( SK, OK ) { if( P.views != nullptr ) \
		hipLaunchKernelGGL(( k_lancp< SK, OK, true > ), \
		dim3( (unsigned) items ), dim3( LP_NT ), lds, st, P ); else \
		hipLaunchKernelGGL(( k_lancp< SK, OK, false > ), \
		dim3( (unsigned) items ), dim3( LP_NT ), lds, st, P ); }
#define LP_OUT( SK ) switch( ok ) { \
		case LP_U8: LP_LAUNCH( SK, LP_U8 ); break; \
		case LP_U16: LP_LAUNCH( SK, LP_U16 ); break; \
		case LP_F16: LP_LAUNCH( SK, LP_F16 ); break; \
		case LP_BF16: LP_LAUNCH( SK, LP_BF16 ); break; \
		default: LP_LAUNCH( SK, LP_F32 ); break; }

	switch( sk )
	{
		case LP_U8: LP_OUT( LP_U8 ); break;
		case LP_U16: LP_OUT( LP_U16 ); break;
		case LP_F16: LP_OUT( LP_F16 ); break;
		case LP_BF16: LP_OUT( LP_BF16 ); break;
		default: LP_OUT( LP_F32 ); break;
	}
#undef LP_OUT
#undef LP_LAUNCH

	up.done( st );
	AVIRHIP_HIPCHECK( hipGetLastError() );
	return( AVIRHIP_OK );
}

} // namespace avirhip
