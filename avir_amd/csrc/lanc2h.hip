// lanc2h.hip -- LANCIR exact 2x RGBA with half / bfloat16 images on either
// side (AVIRHIP_F16, AVIRHIP_BF16 of include/avirhip.h), vertical + horizontal
// Lanczos passes fused in ONE launch over the caller's own images.
//
// The arithmetic is k_lanc2< ..., 4 >'s (lanc2.hip), bit for bit: vertical pass
// first, indices clamped to the frame, no contraction, and on both axes
//   dot6 = ((f0*p0 + f2*p2) + f4*p4) + ((f1*p1 + f3*p3) + f5*p5)
// with the inner float RGBA plan's 32-float coefficient table (lanc2_coef).
// What differs is what moves through HBM. The source is read in the caller's
// own element type and widened exactly in the loader (half: v_cvt_f32_f16,
// denormals included; bfloat16: bits << 16), or it is a float RGBA image -- the
// caller's, or the pack pass's copy of any other source. The result is narrowed
// in the store (half: v_cvt_f16_f32, nearest even, denormals kept -- never the
// pkrtz form; bfloat16: one v_cvt_pk_bf16_f32 per channel pair), behind the
// owner plan's gain ( v * out_mul when the plan is not unity; no clamp: the
// float stage of k_lanc2, IO == 3 ), or it is the float RGBA result -- the
// caller's image when the plan is unity, the plan's `lres` rows otherwise.
//
// Structure: k_lanc2's march (strips of 128 output columns, chunks of source
// rows, 8 source rows per step, a register ring for the 7-row vertical window,
// the step's 16 intermediate rows in LDS as floats, the next step's source
// rows prefetched), with a WHOLE PIXEL per lane on both sides: a workgroup is
// 128 threads,
//   V  one thread per source column (70 px incl. halo): 8 bytes (16-bit
//      elements) or 16 bytes (float) per lane and row from HBM, the ring holds
//      widened pixels; two intermediate rows per source row -> LDS
//      (16 rows x 70 px x 16 B = 17.9 KB, one ds_write_b128 per lane and row)
//   H  one thread per output column: 6 ds_read_b128 + dot6 per output row with
//      the lane's own phase's taps (chosen once, not per row), 16 rows per
//      step, one 8-byte (16-byte: float) store per lane and row
// Row addresses are formed in 64 bits ( base + (long) row * pitch ): no source
// or destination distance limit exists and the host checks none.
//
// Alignment: a pixel is naturally aligned on both sides -- the ONE predicate of
// the routing (api.cpp, lanc_road) and of lanc2h_run's refusal:
//
//   bool lanc2h_image_ok( const void* ptr, int type, long stride )
//   {
//       const size_t px = 4 * dtype_size( type );
//       return(( type == AVIRHIP_F32 || dtype_is_float16_kind( type )) &&
//           ( (uintptr_t) ptr % px ) == 0 && stride > 0 && ( stride & 3 ) == 0 );
//   }
//
// (`stride`: the row pitch in elements.) An image it refuses goes the general
// road: pack pass / float result and output stage.

#include "plan.h"
#include <algorithm>

namespace avirhip {

typedef float lh_f2 __attribute__(( ext_vector_type( 2 )));
typedef float lh_f4 __attribute__(( ext_vector_type( 4 )));
typedef unsigned int lh_u2 __attribute__(( ext_vector_type( 2 )));

#define LH_TW 128                 // output columns per strip
#define LH_NT LH_TW               // threads: one per output pixel
#define LH_RB 8                   // source rows per marching step
#define LH_SW ( LH_TW / 2 + 6 )   // source / intermediate columns incl. halo
// shortest chunk, source rows (8k - 6): a workgroup is two waves, so frames
// under 4 Mpixels need shorter chunks than k_lanc2's 58 rows to fill the chip
// (same process, f16 -> f16 at 58 / 42 / 26 rows: 1080p -> 4K 0.0442 / 0.0349 /
// 0.0294 ms, 720p -> 1440p 0.0436 / 0.0339 / 0.0239, 4K -> 8K 0.0892 / 0.0881 /
// 0.0884; bit-identical)
#define LH_MINQ 26

// element kinds of the kernel's two sides
enum { LH_F32 = 0, LH_F16 = 1, LH_BF16 = 2 };

struct Lanc2hParams
{
	const char* src; long src_pb; // row pitch in bytes
	int sw, sh;
	char* dst; long dst_pb;       // the band's first row; row pitch in bytes
	int dst_row0, nw, nh;
	int srow_lo, srow_hi;
	int nstrips, chunk0, cq;
	const float* coef; // device: [va 6 | vb 6 | pad 4 | ha 6 | hb 6 | pad 4]
	int unity; float out_mul;
};

// a source pixel as it travels from HBM
template< int SRC > struct LhRaw { typedef lh_u2 T; };
template<> struct LhRaw< LH_F32 > { typedef lh_f4 T; };

template< int SRC >
__device__ __forceinline__ lh_f4 lh_widen( const typename LhRaw< SRC > :: T w )
{
	if constexpr( SRC == LH_F32 )
	{
		return( w );
	}
	else
	if constexpr( SRC == LH_F16 )
	{
		// (exact: v_cvt_f32_f16, half denormals kept)
		lh_f4 v;
		v.x = (float) __builtin_bit_cast( _Float16,
			(unsigned short) ( w.x & 0xffffu ));
		v.y = (float) __builtin_bit_cast( _Float16,
			(unsigned short) ( w.x >> 16 ));
		v.z = (float) __builtin_bit_cast( _Float16,
			(unsigned short) ( w.y & 0xffffu ));
		v.w = (float) __builtin_bit_cast( _Float16,
			(unsigned short) ( w.y >> 16 ));
		return( v );
	}
	else
	{
		lh_f4 v;
		v.x = __uint_as_float( w.x << 16 );
		v.y = __uint_as_float( w.x & 0xffff0000u );
		v.z = __uint_as_float( w.y << 16 );
		v.w = __uint_as_float( w.y & 0xffff0000u );
		return( v );
	}
}

// resize4's x86 order (lancir.h:2466-2544): even and odd taps accumulate
// separately.
__device__ __forceinline__ lh_f4 lh_dot6( const float* const f, const lh_f4 p0,
	const lh_f4 p1, const lh_f4 p2, const lh_f4 p3, const lh_f4 p4,
	const lh_f4 p5 )
{
	return((( f[ 0 ] * p0 + f[ 2 ] * p2 ) + f[ 4 ] * p4 ) +
		(( f[ 1 ] * p1 + f[ 3 ] * p3 ) + f[ 5 ] * p5 ));
}

template< int SRC, int OUT >
__global__ void __launch_bounds__( LH_NT ) k_lanc2h( const Lanc2hParams P )
{
	typedef typename LhRaw< SRC > :: T raw_t;
	// intermediate rows of this step, whole pixels: [16][LH_SW]
	__shared__ __attribute__(( aligned( 16 ))) lh_f4 sT[ 2 * LH_RB * LH_SW ];

	// (work items dealt round the 8 XCDs as k_lanc2 deals them)
	const int nwg = gridDim.x;
	const int b = blockIdx.x;
	const int xcd = b & 7;
	const int qd = nwg >> 3;
	const int rm = nwg & 7;
	const int item = ( xcd < rm ? xcd * ( qd + 1 ) :
		rm * ( qd + 1 ) + ( xcd - rm ) * qd ) + ( b >> 3 );

	const int strip = item % P.nstrips;
	const int chunk = P.chunk0 + item / P.nstrips;
	const int tid = threadIdx.x;

	const int qx0 = strip * ( LH_TW / 2 );
	const int qy0 = chunk * P.cq;
	const int qy1 = min( qy0 + P.cq, P.sh );
	const int u0 = qy0 - 3;            // first source row index consumed
	const int nsteps = qy1 - qy0 + 6;  // 6 warm-up rows + chunk rows

	// vertical phase: this thread's source column (threads >= LH_SW idle)
	const bool vact = ( tid < LH_SW );
	const int sx = min( max( qx0 - 3 + tid, 0 ), P.sw - 1 );
	const char* const scol = P.src + (long) sx * (long) sizeof( raw_t );

	// horizontal phase: this thread's output column
	const int xo = qx0 * 2 + tid;
	const bool xok = ( xo < P.nw );
	char* const dcol = P.dst + (long) xo * ( OUT == LH_F32 ? 16 : 8 );
	const int hodd = tid & 1; // odd output column?
	const int ylo = max( qy0 * 2, P.srow_lo );
	const int yhi = min( qy1 * 2, P.srow_hi );

	// the table: uniform loads (scalar registers); the lane's horizontal taps
	// are those of its column's phase
	float va[ 6 ], vb[ 6 ], hf[ 6 ];
#pragma unroll
	for( int i = 0; i < 6; i++ )
	{
		va[ i ] = P.coef[ i ];
		vb[ i ] = P.coef[ 6 + i ];
		hf[ i ] = ( hodd ? P.coef[ 22 + i ] : P.coef[ 16 + i ]);
	}

	lh_f4 ring[ 8 ];
#pragma unroll
	for( int i = 0; i < 8; i++ ) ring[ i ] = (lh_f4) 0.0f;

	raw_t pre[ LH_RB ];

	auto prefetch = [&]( const int ub )
	{
		if( vact )
		{
#pragma unroll
			for( int r = 0; r < LH_RB; r++ )
			{
				const int sy = min( max( ub + r, 0 ), P.sh - 1 );
				pre[ r ] = *(const raw_t*) ( scol + (long) sy * P.src_pb );
			}
		}
	};

	prefetch( u0 );

	for( int sb = 0; sb < nsteps; sb += LH_RB )
	{
		const int ub = u0 + sb;

		// ---- V: 8 source rows -> 16 intermediate rows (ring phase == row & 7)
		if( vact )
		{
#pragma unroll
			for( int rr = 0; rr < LH_RB; rr++ )
			{
				ring[ rr ] = lh_widen< SRC >( pre[ rr ]);
				// rows u-6 .. u of the ring, u = ub + rr
				const lh_f4 m6 = ring[ ( rr - 6 ) & 7 ], m5 = ring[ ( rr - 5 ) & 7 ];
				const lh_f4 m4 = ring[ ( rr - 4 ) & 7 ], m3 = ring[ ( rr - 3 ) & 7 ];
				const lh_f4 m2 = ring[ ( rr - 2 ) & 7 ], m1 = ring[ ( rr - 1 ) & 7 ];
				const lh_f4 m0 = ring[ rr ];
				sT[ ( 2 * rr ) * LH_SW + tid ] = lh_dot6( va, m6, m5, m4, m3, m2,
					m1 );
				sT[ ( 2 * rr + 1 ) * LH_SW + tid ] = lh_dot6( vb, m5, m4, m3, m2,
					m1, m0 );
			}
		}

		AVIRHIP_BARRIER_DRAIN();
		__syncthreads();

		// next step's source rows start their trip from HBM now
		if( sb + LH_RB < nsteps )
		{
			prefetch( ub + LH_RB );
		}

		// ---- H: 16 intermediate rows -> 16 output rows of this strip
		{
			// even output 2q reads columns q-3..q+2 -> local q..q+5;
			// odd output 2q+1 reads q-2..q+3 -> local q+1..q+6
			const lh_f4* const base = &sT[ ( tid >> 1 ) + hodd ];
#pragma unroll 4
			for( int r = 0; r < 2 * LH_RB; r++ )
			{
				const int y = ( ub + ( r >> 1 ) - 3 ) * 2 + ( r & 1 );
				const lh_f4* const t = base + r * LH_SW;
				lh_f4 o = lh_dot6( hf, t[ 0 ], t[ 1 ], t[ 2 ], t[ 3 ], t[ 4 ],
					t[ 5 ]);

				if( xok && y >= ylo && y < yhi )
				{
					char* const q = dcol + (long) ( y - P.dst_row0 ) * P.dst_pb;

					if constexpr( OUT == LH_F32 )
					{
						// (the float result as it is: the gain, where there is
						// one, is the output stage's)
						__builtin_nontemporal_store( o, (lh_f4*) q );
					}
					else
					{
						if( !P.unity )
						{
							o = o * P.out_mul;
						}

						lh_u2 w;

						if constexpr( OUT == LH_F16 )
						{
							// (plain conversions: v_cvt_f16_f32 rounds to nearest
							// even and keeps half denormals)
							const float v0 = o.x, v1 = o.y, v2 = o.z, v3 = o.w;
							const unsigned h0 = __builtin_bit_cast( unsigned short,
								(_Float16) v0 );
							const unsigned h1 = __builtin_bit_cast( unsigned short,
								(_Float16) v1 );
							const unsigned h2 = __builtin_bit_cast( unsigned short,
								(_Float16) v2 );
							const unsigned h3 = __builtin_bit_cast( unsigned short,
								(_Float16) v3 );
							w.x = h0 | ( h1 << 16 );
							w.y = h2 | ( h3 << 16 );
						}
						else
						{
							// (a plain conversion of each pair, v_cvt_pk_bf16_f32:
							// nearest even, float denormals become bfloat16
							// denormals, beyond the largest finite one +-Inf)
							typedef __bf16 bf2 __attribute__(( ext_vector_type( 2 )));
							const lh_f2 lo = { o.x, o.y }, hi = { o.z, o.w };
							w.x = __builtin_bit_cast( unsigned,
								__builtin_convertvector( lo, bf2 ));
							w.y = __builtin_bit_cast( unsigned,
								__builtin_convertvector( hi, bf2 ));
						}

						__builtin_nontemporal_store( w, (lh_u2*) q );
					}
				}
			}
		}

		AVIRHIP_BARRIER_DRAIN();
		__syncthreads();
	}
}

// ---------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------

// The images k_lanc2h reads and stores as they lie: a pixel is naturally
// aligned (`stride`: the row pitch in elements). The ONE test behind the
// routing's promise and lanc2h_run's refusal.
bool lanc2h_image_ok( const void* ptr, int type, long stride )
{
	const size_t px = 4 * dtype_size( type );
	return(( type == AVIRHIP_F32 || dtype_is_float16_kind( type )) &&
		( (uintptr_t) ptr % px ) == 0 && stride > 0 && ( stride & 3 ) == 0 );
}

static int lh_kind( const int type )
{
	return( type == AVIRHIP_F16 ? LH_F16 :
		( type == AVIRHIP_BF16 ? LH_BF16 : LH_F32 ));
}

// Output rows [row0, row1) of the inner plan `q`: RGBA pixels read from `src`,
// the result behind `out`'s gain stored at `out.dst` (the band's first row).
// 1: the call is not this kernel's (float on both sides is k_lanc2's; an image
// the predicate refuses).
int lanc2h_run( const avirhip_plan* q, const ImageRef& src,
	const LancirOut& out, int row0, int row1, hipStream_t st )
{
	const float* const coef = lanc2_coef( q );
	const int sk = lh_kind( src.type );
	const int ok = lh_kind( out.type );

	if( coef == nullptr || q -> l_order != 4 || src.ch != 4 || out.ch != 4 ||
		( sk == LH_F32 && ok == LH_F32 ) ||
		!lanc2h_image_ok( src.ptr, src.type, src.stride ) ||
		!lanc2h_image_ok( out.dst, out.type, out.stride ))
	{
		return( 1 );
	}

	if( row1 <= row0 )
	{
		return( AVIRHIP_OK );
	}

	Lanc2hParams P;
	P.src = (const char*) src.ptr;
	P.src_pb = src.stride * (long) dtype_size( src.type );
	P.sw = q -> src_w; P.sh = q -> src_h;
	P.dst = (char*) out.dst;
	P.dst_pb = out.stride * (long) dtype_size( out.type );
	P.dst_row0 = row0; P.nw = q -> new_w; P.nh = q -> new_h;
	P.srow_lo = row0; P.srow_hi = row1;
	P.nstrips = ( q -> new_w + LH_TW - 1 ) / LH_TW;
	P.coef = coef;
	P.unity = ( ok == LH_F32 ? 1 : out.unity );
	P.out_mul = out.out_mul;

	// k_lanc2's chunk rule with a floor of its own: chunk = 8k - 6 source rows
	// (6 warm-up rows per chunk); fill whole rounds of 256 CUs x 8 resident
	// workgroups (LDS) with chunks of >= LH_MINQ rows
	const int slots = 256 * 8;
	int cq = 0;

	for( int rounds = 1; rounds <= 8 && cq == 0; rounds++ )
	{
		const int nch = std::max( 1, rounds * slots / P.nstrips );
		int c = ( q -> src_h + nch - 1 ) / nch;
		c = (( c + 6 + LH_RB - 1 ) / LH_RB ) * LH_RB - 6;

		if( c >= LH_MINQ || rounds == 8 )
		{
			cq = std::max( c, LH_MINQ );
		}
	}

	// (k_lanc2's knob and rounding, read per call: sweeps and the seam tests)
	const char* ecq = getenv( "AVIRHIP_LANC2_CQ" );

	if( ecq != nullptr && atoi( ecq ) >= 2 )
	{
		cq = (( atoi( ecq ) + 6 + LH_RB - 1 ) / LH_RB ) * LH_RB - 6;
	}

	P.cq = cq;
	const int cr = cq * 2;
	P.chunk0 = row0 / cr;
	const int chunk1 = ( row1 - 1 ) / cr;
	const int items = P.nstrips * ( chunk1 - P.chunk0 + 1 );

	if( getenv( "AVIRHIP_VERBOSE" ) != nullptr )
	{
		fprintf( stderr, "k_lanc2h: %d items (strips %d, cq %d, chunk0 %d)\n",
			items, P.nstrips, P.cq, P.chunk0 );
	}

#define LH_LAUNCH( SK, OK ) hipLaunchKernelGGL(( k_lanc2h< SK, OK > ), \
		dim3( items ), dim3( LH_NT ), 0, st, P )

	switch( sk * 3 + ok )
	{
		case LH_F32 * 3 + LH_F16: LH_LAUNCH( LH_F32, LH_F16 ); break;
		case LH_F32 * 3 + LH_BF16: LH_LAUNCH( LH_F32, LH_BF16 ); break;
		case LH_F16 * 3 + LH_F32: LH_LAUNCH( LH_F16, LH_F32 ); break;
		case LH_F16 * 3 + LH_F16: LH_LAUNCH( LH_F16, LH_F16 ); break;
		case LH_F16 * 3 + LH_BF16: LH_LAUNCH( LH_F16, LH_BF16 ); break;
		case LH_BF16 * 3 + LH_F32: LH_LAUNCH( LH_BF16, LH_F32 ); break;
		case LH_BF16 * 3 + LH_F16: LH_LAUNCH( LH_BF16, LH_F16 ); break;
		default: LH_LAUNCH( LH_BF16, LH_BF16 ); break;
	}
#undef LH_LAUNCH

	AVIRHIP_HIPCHECK( hipGetLastError() );
	return( AVIRHIP_OK );
}

} // namespace avirhip
