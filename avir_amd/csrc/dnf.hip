// dnf.hip -- integer-ratio downsizing (cfg4 of BASELINE.json: 3x; also 2x), both
// axes in ONE marching launch: the horizontally resized intermediate (the
// reference's FltBuf, avir.h:4880-4979) never exists in memory.
//
// What the plan looks like (see dn.hip), per axis, (K, NT) = (2, 24) or (3, 38):
//   T[j] = 0 + sum_{t<NT} c[t] * S[clamp(K*j + c0 + t)]      (doResize,
//          avir.h:3884-4096, one bank phase)
//   O[j] = f0*T[j] + sum_{i=1..3} f_i*(T[clamp(j+i)] + T[clamp(j-i)])
//          (correction filter, doFilter avir.h:3748-3866)
// horizontal axis first (every source row -> one FltBuf row F), then the same
// along y over the F rows.
//
// Work item = strip of 42 output columns x chunk of output rows, one workgroup
// of 12 waves with two ROLES marching down the chunk's source rows 16 at a time:
//
//   8 "row" waves     each owns 2 source rows of the step. Its row segments
//       arrive by LDS-DMA one step ahead into wave-private buffers (loads
//       retire in order: vmcnt counts them across the barriers). Lane =
//       (row, triple of resize outputs, half pixel): R = 3 consecutive T
//       outputs accumulate in registers from ONE pass over NT + 2K inputs
//       (ds_read_b64 at compile-time offsets, lane stride 3K pixels: bank-
//       conflict free for K = 3; for K = 2 the DMA lands even and odd pixels
//       in two planes, which makes the stride 3 slots again), then the FIR7
//       along x -> one F row per source row into an LDS ring of 2 x 16 rows.
//   4 "column" waves  lane = ONE channel of one pixel column. Streaming
//       accumulation along y: a lane multiplies each new F value into the
//       ceil(NT/K) output rows alive at it (16 accumulator slots, static:
//       the row loop is unrolled over the 16-output period), every sum starts
//       from +0.0f and receives its taps in ascending order; a finished T row
//       enters an 8-slot register window and the FIR7 along y produces one
//       output row, stored straight to the destination (or through the
//       integer output stage). F rows of step s are consumed during step
//       s + 1: one s_barrier per step, nobody waits inside a step.
//
// Each SIMD hosts two row waves (packed multiplies / adds with the tap as an
// SGPR-pair half, op_sel) and one column wave (scalar v_mul / v_add with SGPR
// taps): equal vector-ALU time per step by construction (K = 3: 2 x 258 packed
// + 490 scalar instructions).
//
// Cost of the chunking: a chunk's first output row needs NT + 5K source rows
// before it, its strip 6 extra T columns -- (1 + 53/270) x (48/42) on the
// horizontal arithmetic for cfg4 with one workgroup per compute unit.
//
// Arithmetic contract: -ffp-contract=off, mul then add in the reference's tap
// order => bit-identical to the two-pass kernels and to the reference.
//
// The march is written once, df_march, over the KIND of the pixels on each side
// (how a row wave gets a source pixel into its row buffer, how a column wave's
// lane stores its value: "source and store kinds" below). Two kernels call it:
// k_dnf, float RGBA rows on both sides, with the timing ablations and in-kernel
// clocks of AVIRHIP_DNF_DBG; k_dnfh, every other pair of kinds, without them.

#include "gpass_dev.h"
#include "dn_dev.h"
#include "dnf_dev.h"
#include <algorithm>
#include <string.h>
#include <stdlib.h>
#include <stdio.h>
#include <vector>
#include "dnsrgb_dev.h"
namespace avirhip {

#define DF_W 42     // output columns per strip
#define DF_NT1 48   // resize (T) outputs per row: 16 triples
// 12 waves per workgroup: NHW row waves + the column waves of the strip's 168
// elements. 8 + 4 (42 elements each): 16 rows per step, every SIMD hosts two
// row waves and a column wave. 9 + 3 (56 each): 18 rows per step, one SIMD
// hosts three row waves instead -- the column waves' share of the vector ALU
// shrinks with their idle lanes (K = 3: 209 -> 194 SIMD cycles per row), at
// the price of a longer static unroll of the column waves (the step must
// divide a whole number of 16-output periods: 8 phases instead of 3).
#define DF_NTHR 768
#define DF_MAXRS 18

struct DnFParams
{
	DnAxisP H, V;
	const float* src; long src_ss;  // elements per source row
	float* dst; long dst_ss;        // float RGBA rows, row dst_row0 at dst
	int dst_row0;
	int row_lo, row_hi;             // output rows to store
	int nstrips, nchunks, crows;    // work items, strip fastest; rows per chunk
	GPOut out;                      // on != 0: integer output stage in the store
	unsigned long long* clk;        // dbg & 16: per wave {total, dma wait, barrier
	                                // wait, 0} shader clocks
	int dbg;                        // timing ablations (AVIRHIP_DNF_DBG): 1 no
	                                // column arithmetic, 2 no row arithmetic,
	                                // 4 no source loads, 8 no FIR in the row waves
};

// one element (a lane's channel of its pixel, byte offset `voff` inside the
// row) through the integer output stage (gp_store_int's arithmetic per
// channel); row `row` of the caller's band
__device__ __forceinline__ void df_store_elem( const GPOut& O,
	const __amdgpu_buffer_rsrc_t rs, const int voff, const int row,
	const float v )
{
	if( O.type == AVIRHIP_F32 )
	{
		__builtin_amdgcn_raw_buffer_store_b32( __builtin_bit_cast( unsigned,
			v ), rs, voff, row * (int) O.stride * 4, 0 );
		return;
	}

	float t = v;
	float a = v;

	if( O.use_tr )
	{
		a = t * O.tr_muli;
		t = (float) (int) ( a + 0.5f ) * O.tr_mul;
	}
	else
	{
		t = (float) (int) ( t + 0.5f );
	}

	t = fminf( fmaxf( t, 0.0f ), O.pk_out );
	t = avirhip_x86_round_fix( a, t, O.pk_out );
	const unsigned int q = (unsigned int) t;

	if( O.type == AVIRHIP_U8 )
	{
		__builtin_amdgcn_raw_buffer_store_b8( (unsigned char) q, rs, voff,
			row * (int) O.stride, 0 );
	}
	else
	{
		__builtin_amdgcn_raw_buffer_store_b16( (unsigned short) q, rs, voff,
			row * (int) O.stride * 2, 0 );
	}
}

// input i of a lane's three outputs: tap i - K * r of output r
template< int K, int NT, int I >
__device__ __forceinline__ void df_feed( f2 ( &acc )[ 3 ], const f2 v,
	const f2 ( &cp )[ NT / 2 ])
{
	constexpr int t0 = I, t1 = I - K, t2 = I - 2 * K;
	constexpr bool v0 = ( t0 >= 0 && t0 < NT );
	constexpr bool v1 = ( t1 >= 0 && t1 < NT );
	constexpr bool v2 = ( t2 >= 0 && t2 < NT );

	if constexpr( v0 && v1 && v2 )
	{
		df_pk3< ( t0 & 1 ) | (( t1 & 1 ) << 1 ) | (( t2 & 1 ) << 2 ) >(
			acc[ 0 ], acc[ 1 ], acc[ 2 ], v, cp[ t0 >> 1 ], cp[ t1 >> 1 ],
			cp[ t2 >> 1 ]);
	}
	else if constexpr( v0 && v1 )
	{
		df_pk2< ( t0 & 1 ) | (( t1 & 1 ) << 1 ) >( acc[ 0 ], acc[ 1 ], v,
			cp[ t0 >> 1 ], cp[ t1 >> 1 ]);
	}
	else if constexpr( v1 && v2 )
	{
		df_pk2< ( t1 & 1 ) | (( t2 & 1 ) << 1 ) >( acc[ 1 ], acc[ 2 ], v,
			cp[ t1 >> 1 ], cp[ t2 >> 1 ]);
	}
	else if constexpr( v0 )
	{
		df_pk1< ( t0 & 1 ) >( acc[ 0 ], v, cp[ t0 >> 1 ]);
	}
	else if constexpr( v2 )
	{
		df_pk1< ( t2 & 1 ) >( acc[ 2 ], v, cp[ t2 >> 1 ]);
	}
	else
	{
		static_assert( !v1, "NT >= 2K: a lone middle tap cannot happen" );
	}
}

// ---- column waves: one asm statement per F row.
// A lane keeps the 16 accumulator slots (output j lives in slot j % 16) as 8
// register PAIRS {slot 4q + b, slot 4q + b + 2}: the two outputs of a pair,
// j - 2 and j, are at taps t + 2K and t of the same row, so ONE packed
// multiply (the F value broadcast, times the register pair V2[t + 2K] =
// {c[t + 2K], c[t]}) and one packed add serve both. V2 is c[] laid out for
// that, with zeros where a pair's other output is not alive (the table has
// NT + 2K entries): a dead half receives +-0 products, and every slot is
// zeroed on the row its next output starts at. A wave issues an instruction
// every ~4 cycles whatever it is, and the column waves are the workgroup's
// longest instruction streams: 13 taps = 26 scalar instructions become 14-16.
// The F values arrive as pairs of rows {row 2m, row 2m + 1} (ds_read2_b32):
// RSEL picks the half.
#define DF_RSEL0 "op_sel:[0,0] op_sel_hi:[0,1]"
#define DF_RSEL1 "op_sel:[1,0] op_sel_hi:[1,1]"
#define DF_VP_MULR0( i ) \
	"v_pk_mul_f32 %[q" #i "], %[vp], %[k" #i "] " DF_RSEL0 "\n\t"
#define DF_VP_MULR1( i ) \
	"v_pk_mul_f32 %[q" #i "], %[vp], %[k" #i "] " DF_RSEL1 "\n\t"
#define DF_VP_ADD( i ) "v_pk_add_f32 %[a" #i "], %[a" #i "], %[q" #i "]\n\t"
#define DF_VP_OUT( i ) [a##i] "+v"( a##i ), [q##i] "=&v"( q##i ),
#define DF_VP_IN( i ) [k##i] "v"( k##i ),
// pairs 1 .. N-1 (pair 0 closes the operand lists: no trailing comma)
#define DF_PR6( M ) M( 1 ) M( 2 ) M( 3 ) M( 4 ) M( 5 )
#define DF_PR7( M ) DF_PR6( M ) M( 6 )
#define DF_PR8( M ) DF_PR7( M ) M( 7 )
#define DF_VSTMT( PR, MULR ) asm volatile( \
	MULR( 0 ) PR( MULR ) DF_VP_ADD( 0 ) PR( DF_VP_ADD ) \
	: PR( DF_VP_OUT ) [a0] "+v"( a0 ), [q0] "=&v"( q0 ) \
	: PR( DF_VP_IN ) [k0] "v"( k0 ), [vp] "v"( vp ))

template< int N, int R >
__device__ __forceinline__ void df_vstmt( f2& a0, f2& a1, f2& a2, f2& a3,
	f2& a4, f2& a5, f2& a6, f2& a7, const f2 vp, const f2 k0, const f2 k1,
	const f2 k2, const f2 k3, const f2 k4, const f2 k5, const f2 k6,
	const f2 k7 )
{
	f2 q0, q1, q2, q3, q4, q5, q6, q7;

	if constexpr( N == 8 && R == 0 ) DF_VSTMT( DF_PR8, DF_VP_MULR0 );
	else if constexpr( N == 8 && R == 1 ) DF_VSTMT( DF_PR8, DF_VP_MULR1 );
	else if constexpr( N == 7 && R == 0 ) DF_VSTMT( DF_PR7, DF_VP_MULR0 );
	else if constexpr( N == 7 && R == 1 ) DF_VSTMT( DF_PR7, DF_VP_MULR1 );
	else if constexpr( N == 6 && R == 0 ) DF_VSTMT( DF_PR6, DF_VP_MULR0 );
	else if constexpr( N == 6 && R == 1 ) DF_VSTMT( DF_PR6, DF_VP_MULR1 );
	else
	{
		static_assert( N < 0, "6-8 pair registers are alive at a row" );
	}
}

// Row U of the 16-output period: the pair registers with an output alive and
// their V2 entries; the slot (if any) whose output starts at this row.
template< int K, int NT, int U >
struct DfRow
{
	int n;
	int pi[ 8 ], vi[ 8 ];
	int zslot; // -1: none

	constexpr DfRow() : n( 0 ), pi(), vi(), zslot( -1 )
	{
		for( int r = 0; r < 8; r++ )
		{
			const int slo = ( r >> 1 ) * 4 + ( r & 1 ), shi = slo + 2;
			int tlo = -1, thi = -1;

			// the alive outputs are j = U / K, U / K - 1, ... (tap U - K * j)
			for( int d = 0; d < 16; d++ )
			{
				const int j = U / K - d;
				const int t = U - K * j;

				if( t >= 0 && t < NT )
				{
					const int sl = (( j % 16 ) + 16 ) % 16;
					if( sl == slo ) tlo = t;
					if( sl == shi ) thi = t;
					if( t == 0 ) zslot = sl;
				}
			}

			if( tlo >= 0 || thi >= 0 )
			{
				pi[ n ] = r;
				vi[ n ] = ( thi >= 0 ? thi + 2 * K : tlo );
				n++;
			}
		}
	}
};

template< int K, int NT, int B, int I0 >
__device__ __forceinline__ void df_feed_batch( f2 ( &acc )[ 3 ],
	const DfBatch< B >& d, const f2 ( &cp )[ NT / 2 ])
{
	dn_static_for< B >( [&]( auto jc )
	{
		constexpr int j = decltype( jc )::value;
		df_feed< K, NT, I0 + j >( acc, d.v[ j ], cp );
	} );
}

// ---------------------------------------------------------------------
// source and store kinds
// ---------------------------------------------------------------------
//
// The march's row and column roles, strips, chunks and tap order (the head of
// this file) are the same for every kind; a kind decides
//   SRC  DH_F32: float RGBA rows, by LDS-DMA one step ahead.
//        DH_F16 / DH_BF16: the row waves read the caller's 16-bit RGBA rows
//        where they lie. LDS-DMA has no 8-byte form, so a lane takes its pixel
//        of each piece with ONE 8-byte buffer load into registers, issued one
//        step ahead where a float source issues the DMA (2 rows x NPH pieces
//        x 2 VGPRs), and at the head of the step widens it exactly (half:
//        v_cvt_f32_f16, denormals kept; bfloat16: bits << 16) and writes it
//        with one ds_write_b128 into the slot of sS the DMA would have filled
//        (lane l of piece q: slot q * 64 + l -- for K = 2 that IS df_slot's
//        even / odd plane layout, the lane's pixel being 2 l + q). The row
//        buffers are wave-private: an lgkmcnt wait between the writes and the
//        window reads, no barrier. Everything behind sS is the same.
//   OUT  DH_F32: float RGBA rows, or the integer output stage (df_store_elem).
//        DH_F16 / DH_BF16: a column wave's lane narrows its channel (half:
//        v_cvt_f16_f32, nearest even, never the pkrtz form; bfloat16:
//        v_cvt_pk_bf16_f32, low half) and stores 2 bytes at
//        ( x * ch + c ) * 2 of the caller's row.
//
// With sRGB gamma (DnSParams; dnsrgb_dev.h has the stages' expressions):
//   SRC  DH_S8: the caller's uint8 RGBA rows. ONE 4-byte buffer load per
//        pixel, issued a step ahead like the 8-byte ones; at the head of the
//        step the lane linearises it -- tbl[ v ] per colour channel from an
//        LDS copy of the plan's 256-entry table, (float) v * gm for the alpha
//        channel -- and writes the slot of sS: the pack pass's float pixel.
//   OUT  DH_S8: a uint8 result of 1-4 channels. A column wave's lane counts
//        the thresholds <= its value (k_epilogue_gamma_thr's eight compares
//        over an LDS copy of the plan's 2 x 256 thresholds; the step's 6 or 8
//        outputs are searched level by level, so a level's LDS reads are
//        independent of each other) and stores one byte at x * ch + c.
//        Values outside |v| <= 16 take that kernel's direct expression.
//   A workgroup fills its tables once, before its first step, behind a
//   barrier of their own. Pairs: (S8, S8), (S8, F32), (F32, S8).
enum { DH_F32 = 0, DH_F16 = 1, DH_BF16 = 2, DH_S8 = 3 };

// DnFParams and the gamma stages' parameters: the kernels with a DH_S8 side
struct DnSParams
{
	DnFParams F;
	DnGamma G;
};

__device__ __forceinline__ const DnFParams& dh_core( const DnFParams& p )
{
	return( p );
}

__device__ __forceinline__ const DnFParams& dh_core( const DnSParams& p )
{
	return( p.F );
}

template< int SRC, int OUT >
struct DhParams
{
	typedef DnFParams type;
};

template< int OUT >
struct DhParams< DH_S8, OUT >
{
	typedef DnSParams type;
};

template<>
struct DhParams< DH_F32, DH_S8 >
{
	typedef DnSParams type;
};

typedef unsigned int dh_u2 __attribute__(( ext_vector_type( 2 )));

// a lane's uint8 RGBA pixel of one piece: dh_ld8's addressing and discipline
__device__ __forceinline__ void dh_ld4( unsigned int& r,
	const __amdgpu_buffer_rsrc_t rs, const int voff, const unsigned soff )
{
	asm volatile( "buffer_load_dword %0, %1, %2, %3 offen"
		: "+v"( r ) : "v"( voff ), "s"( rs ), "s"( soff ) : "memory" );
}

// the pack pass's float pixel of a uint8 RGBA pixel (k_pack_gamma_px< uint8_t,
// 4 >): `tbl` the LDS copy of the table, `ai` the alpha channel (0, 3, or
// neither)
__device__ __forceinline__ f4 dh_linear( const unsigned int w,
	const float* const tbl, const int ai, const float gm )
{
	f4 v;
	v.x = tbl[ w & 255u ];
	v.y = tbl[ ( w >> 8 ) & 255u ];
	v.z = tbl[ ( w >> 16 ) & 255u ];
	v.w = tbl[ w >> 24 ];

	if( ai == 0 )
	{
		v.x = (float) ( w & 255u ) * gm;
	}

	if( ai == 3 )
	{
		v.w = (float) ( w >> 24 ) * gm;
	}

	return( v );
}

// a lane's pixel of one piece: 8 bytes at voff + soff (gp_dma's addressing),
// into registers the caller waits for (AVIRHIP_WAITCNT_VM) before it reads
// them -- tied operand: to the compiler the registers are one value from the
// first load on, nothing copies them while a load is in flight
__device__ __forceinline__ void dh_ld8( dh_u2& r,
	const __amdgpu_buffer_rsrc_t rs, const int voff, const unsigned soff )
{
	asm volatile( "buffer_load_dwordx2 %0, %1, %2, %3 offen"
		: "+v"( r ) : "v"( voff ), "s"( rs ), "s"( soff ) : "memory" );
}

template< int SRC >
__device__ __forceinline__ f4 dh_widen( const dh_u2 w )
{
	f4 v;

	if constexpr( SRC == DH_F16 )
	{
		// (exact: v_cvt_f32_f16, half denormals kept)
		v.x = (float) __builtin_bit_cast( _Float16,
			(unsigned short) ( w.x & 0xffffu ));
		v.y = (float) __builtin_bit_cast( _Float16,
			(unsigned short) ( w.x >> 16 ));
		v.z = (float) __builtin_bit_cast( _Float16,
			(unsigned short) ( w.y & 0xffffu ));
		v.w = (float) __builtin_bit_cast( _Float16,
			(unsigned short) ( w.y >> 16 ));
	}
	else
	{
		v.x = __builtin_bit_cast( float, w.x << 16 );
		v.y = __builtin_bit_cast( float, w.x & 0xffff0000u );
		v.z = __builtin_bit_cast( float, w.y << 16 );
		v.w = __builtin_bit_cast( float, w.y & 0xffff0000u );
	}

	return( v );
}

// one pixel into a row buffer (byte address `ad` + OFF)
template< int OFF >
__device__ __forceinline__ void dh_st16( const unsigned ad, const f4 v )
{
	asm volatile( "ds_write_b128 %0, %1 offset:%2"
		:: "v"( ad ), "v"( v ), "i"( OFF ) : "memory" );
}

// the narrowing contract of avirhip.h, one element
template< int OUT >
__device__ __forceinline__ unsigned short dh_narrow( const float v )
{
	if constexpr( OUT == DH_F16 )
	{
		return( __builtin_bit_cast( unsigned short, (_Float16) v ));
	}
	else
	{
		return( __builtin_bit_cast( unsigned short, (__bf16) v ));
	}
}

// the registers of a step's loads (dh_u2 or unsigned int each), once all of
// them have returned
template< class T, int NP >
__device__ __forceinline__ void dh_wait_raw( T ( &r )[ 2 ][ NP ])
{
	static_assert( NP == 2 || NP == 3, "pieces per row" );

	if constexpr( NP == 3 )
	{
		asm volatile( AVIRHIP_WAITCNT_VM( 0 )
			: "+v"( r[ 0 ][ 0 ]), "+v"( r[ 0 ][ 1 ]), "+v"( r[ 0 ][ 2 ]),
			"+v"( r[ 1 ][ 0 ]), "+v"( r[ 1 ][ 1 ]), "+v"( r[ 1 ][ 2 ])
			:: "memory" );
	}
	else
	{
		asm volatile( AVIRHIP_WAITCNT_VM( 0 )
			: "+v"( r[ 0 ][ 0 ]), "+v"( r[ 0 ][ 1 ]), "+v"( r[ 1 ][ 0 ]),
			"+v"( r[ 1 ][ 1 ]) :: "memory" );
	}
}

// the level-by-level threshold search of a column wave's step: N values, each
// the count of thresholds t[ 1 .. 255 ] <= v (k_epilogue_gamma_thr's compares)
template< int N >
__device__ __forceinline__ void dh_count( int ( &lo )[ N ],
	const float ( &v )[ N ], const float* const t )
{
#pragma unroll
	for( int k = 0; k < N; k++ )
	{
		lo[ k ] = 0;
	}

#pragma unroll
	for( int s = 128; s >= 1; s >>= 1 )
	{
		float th[ N ];
#pragma unroll
		for( int k = 0; k < N; k++ )
		{
			th[ k ] = t[ lo[ k ] + s ];
		}

#pragma unroll
		for( int k = 0; k < N; k++ )
		{
			lo[ k ] += ( v[ k ] >= th[ k ] ? s : 0 );
		}
	}
}

// a workgroup's LDS copies of the plan's tables: threads 0-255 the
// linearising table (a DH_S8 source), threads 256-767 the thresholds (a DH_S8
// result); the caller's barrier hands them over
template< int SRC, int OUT >
__device__ __forceinline__ void dh_fill_tables( const DnGamma& G,
	const int tid )
{
	static_assert( DF_NTHR == 768, "one table element per thread" );

	if constexpr( SRC == DH_S8 )
	{
		if( tid < 256 )
		{
			ds_table< 256 >()[ tid ] = G.tbl[ tid ];
		}
	}

	if constexpr( OUT == DH_S8 )
	{
		if( tid >= 256 )
		{
			ds_table< 512 >()[ tid - 256 ] = G.thr[ tid - 256 ];
		}
	}
}

// ---------------------------------------------------------------------
// the march
// ---------------------------------------------------------------------

// (instrumented barrier / wait: the clocks only tick when dbg & 16)
#define DF_TIMED( acc, stmt ) do { if( dbg & 16 ) { \
	const unsigned long long t0_ = __builtin_readcyclecounter(); stmt; \
	acc += __builtin_readcyclecounter() - t0_; } else { stmt; } } while( 0 )

// A workgroup's whole march, for the kernels below to call. SRC, OUT: the kinds
// above; PT: DnFParams, or DnSParams with a DH_S8 side. DBG: the timing
// ablations of DnFParams::dbg and the in-kernel clocks are in the code; without
// it `dbg` is the constant 0 and none of them is.
template< int KH, int NTH, int KV, int NTV, int DF_NHW, int SRC, int OUT,
	bool DBG, class PT >
__device__ __forceinline__ void df_march( const PT& PA )
{
	constexpr bool S8 = ( SRC == DH_S8 || OUT == DH_S8 );
	const DnFParams& P = dh_core( PA );
	const int dbg = ( DBG ? P.dbg : 0 );
	unsigned long long tk_total = ( dbg & 16 ? __builtin_readcyclecounter() :
		0 ), tk_dma = 0, tk_bar = 0;
	constexpr int DF_NVW = 12 - DF_NHW;         // column waves
	constexpr int DF_RS = 2 * DF_NHW;           // source rows per step
	constexpr int DF_LPV = DF_W * 4 / DF_NVW;   // elements per column wave
	// phases of the column waves' unroll: steps per whole number of periods
	constexpr int DF_NPH = ( DF_RS == 16 ? KV : ( KV == 3 ? 8 : 16 ));
	static_assert( DF_NVW * DF_LPV == DF_W * 4 && ( DF_NPH * DF_RS ) %
		( 16 * KV ) == 0, "column wave geometry" );
	constexpr int NPH = ( KH * ( DF_NT1 - 1 ) + NTH + 63 ) / 64; // DMA pieces
	constexpr int ROWPX = NPH * 64;
	constexpr int NIN = NTH + 2 * KH; // inputs of a lane's three outputs
	constexpr int BI = NIN / 4;       // ... in four batches
	static_assert( KH != 2 || NPH == 2, "plane layout assumes two pieces" );
	static_assert(( NTH & 1 ) == 0 && BI * 4 == NIN, "tap pairs, batches" );

	__shared__ __attribute__(( aligned( 16 ))) f4
		sS[ DF_NHW ][ 2 ][ 2 ][ ROWPX ];
	__shared__ __attribute__(( aligned( 16 ))) f4 sT[ DF_NHW ][ 2 ][ DF_NT1 ];
	__shared__ __attribute__(( aligned( 16 ))) float
		sF[ 2 ][ DF_RS ][ DF_W * 4 ];

	const int tid = threadIdx.x;
	const int lane = tid & 63;
	const int wave = __builtin_amdgcn_readfirstlane( tid >> 6 );

	// XCD-aware dealing (workgroup b runs on XCD b % 8): an XCD's contiguous
	// item range holds whole chunk-rows of strips, so x-neighbours, which
	// share 53 of their source columns, share an L2
	const int nwg = gridDim.x;
	const int b = blockIdx.x;
	const int xcd = b & 7;
	const int qd = nwg >> 3;
	const int rm = nwg & 7;
	const int item = ( xcd < rm ? xcd * ( qd + 1 ) :
		rm * ( qd + 1 ) + ( xcd - rm ) * qd ) + ( b >> 3 );

	const int chunk = item / P.nstrips;
	const int strip = item - chunk * P.nstrips;

	// output rows of this chunk, the T rows (j) they need, the source rows
	const int oy0 = P.row_lo + chunk * P.crows;
	const int oy1 = min( oy0 + P.crows, P.row_hi );
	const int vlast = P.V.out_len - 1;
	const bool top = ( oy0 - 3 < 0 );
	const int jstart = max( oy0 - 3, 0 );
	const int n_u = oy1 + 3 - jstart;
	const int n_rows = KV * ( n_u - 1 ) + NTV;
	const int S = ( n_rows + DF_RS - 1 ) / DF_RS;
	const int r_first = KV * jstart + P.V.c0;

	if( wave < DF_NHW )
	{
		// ------------------------------------------------------------
		// row waves
		// ------------------------------------------------------------
		const int h = wave;
		// (constant address space: scalar loads, the taps are SGPR operands)
		gp_cfloat* const hc = (gp_cfloat*) P.H.coef;
		f2 cp[ NTH / 2 ];
#pragma unroll
		for( int m = 0; m < NTH / 2; m++ )
		{
			cp[ m ].x = hc[ 2 * m ];
			cp[ m ].y = hc[ 2 * m + 1 ];
		}

		const float f0 = hc[ NTH ], f1 = hc[ NTH + 1 ], f2_ = hc[ NTH + 2 ],
			f3 = hc[ NTH + 3 ];

		const int rho = lane >> 5;        // which of the wave's two rows
		const int tri = ( lane & 31 ) >> 1;
		const int hf = lane & 1;
		const int X0 = strip * DF_W - 3;  // first T output of the strip
		const int in0 = KH * X0 + P.H.c0; // its first input pixel
		const int olast = P.H.out_len - 1;
		const bool edge = ( X0 < 0 || X0 + DF_NT1 - 1 > olast );

		// per-lane source columns of the DMA pieces (clamped: the extended
		// view), the same for every row
		int voff[ NPH ];
#pragma unroll
		for( int q = 0; q < NPH; q++ )
		{
			const int px = ( KH == 2 ? lane * 2 + q : q * 64 + lane );
			voff[ q ] = dn_clampi( in0 + px, P.H.in_len - 1 ) *
				( SRC == DH_F32 ? 16 : ( SRC == DH_S8 ? 4 : 8 ));
		}

		const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
			(void*) P.src, 0, 0x7fffffff, 0x00020000 );

		const unsigned row_b = (unsigned) P.src_ss *
			( SRC == DH_F32 ? 4u : ( SRC == DH_S8 ? 1u : 2u ));
		const unsigned lds_s = (unsigned) (unsigned long) (lds_char*)
			&sS[ h ][ 0 ][ 0 ][ 0 ];

		// LDS byte address of this lane's first input in buffer 0
		const unsigned lds_in = lds_s + ( rho * ROWPX +
			( KH == 2 ? 3 : 9 ) * tri ) * 16 + hf * 8;

		const int vin_last = P.V.in_len - 1;

		// a 16-bit or uint8 source: the lane's pixels of the step ahead, as
		// loaded
		typedef typename std::conditional< SRC == DH_S8, unsigned int,
			dh_u2 >::type raw_t;
		raw_t raw[ 2 ][ NPH ];
#pragma unroll
		for( int rr = 0; rr < 2; rr++ )
		{
#pragma unroll
			for( int q = 0; q < NPH; q++ )
			{
				raw[ rr ][ q ] = (raw_t) 0u;
			}
		}

		// the slot of buffer 0, row 0, piece 0 this lane fills
		const unsigned lds_w = lds_s + lane * 16;

		auto issue = [&]( const int s )
		{
			const int bf = s & 1;
#pragma unroll
			for( int rr = 0; rr < 2; rr++ )
			{
				const int row = dn_clampi( r_first + s * DF_RS + 2 * h + rr,
					vin_last );
				const unsigned soff = (unsigned) row * row_b;
#pragma unroll
				for( int q = 0; q < NPH; q++ )
				{
					if constexpr( SRC == DH_F32 )
					{
						df_dma( rsrc, lds_s + (( bf * 2 + rr ) * ROWPX +
							q * 64 ) * 16, voff[ q ], soff );
					}
					else
					if constexpr( SRC == DH_S8 )
					{
						dh_ld4( raw[ rr ][ q ], rsrc, voff[ q ], soff );
					}
					else
					{
						dh_ld8( raw[ rr ][ q ], rsrc, voff[ q ], soff );
					}
				}
			}
		};

		issue( 0 );

		// (the tables, behind the first step's loads: every wave of the
		// workgroup fills its share, one barrier hands them over)
		if constexpr( S8 )
		{
			dh_fill_tables< SRC, OUT >( PA.G, tid );
			__syncthreads();
		}

		for( int s = 0; s < S; s++ )
		{
			const int bf = s & 1;

			if constexpr( SRC == DH_F32 )
			{
				if( s + 1 < S )
				{
					if( !( dbg & 4 ))
					issue( s + 1 );

					if( NPH == 3 )
					{
						DF_TIMED( tk_dma, GP_WAIT_VM( 6 ));
					}
					else
					{
						DF_TIMED( tk_dma, GP_WAIT_VM( 4 ));
					}
				}
				else
				{
					DF_TIMED( tk_dma, GP_WAIT_VM( 0 ));
				}
			}
			else
			{
				// this step's pixels have landed in the registers (the only
				// vector-memory loads of a row wave in flight are theirs):
				// widen, write the slots, send for the next step's
				dh_wait_raw( raw );
				const unsigned wad = lds_w + bf * ( 2 * ROWPX * 16 );
#pragma unroll
				for( int q = 0; q < NPH; q++ )
				{
					if constexpr( SRC == DH_S8 )
					{
						const float* const tb = ds_table< 256 >();
						dh_st16< 0 >( wad + q * 1024, dh_linear( raw[ 0 ][ q ],
							tb, PA.G.alpha_index, PA.G.gm ));
						dh_st16< ROWPX * 16 >( wad + q * 1024, dh_linear(
							raw[ 1 ][ q ], tb, PA.G.alpha_index, PA.G.gm ));
					}
					else
					{
						dh_st16< 0 >( wad + q * 1024,
							dh_widen< SRC >( raw[ 0 ][ q ]));
						dh_st16< ROWPX * 16 >( wad + q * 1024,
							dh_widen< SRC >( raw[ 1 ][ q ]));
					}
				}

				if( s + 1 < S )
				{
					issue( s + 1 );
				}

				// (wave-private buffers: the writes before the window reads)
				AVIRHIP_WAIT_LGKM( 0 );
			}

			// ---- resize: 3 consecutive outputs per lane
			if( !( dbg & 2 ))
			{
				const unsigned ad = lds_in + bf * ( 2 * ROWPX * 16 );
				DfBatch< BI > d0, d1, d2, d3;
				f2 acc[ 3 ];
				acc[ 0 ] = (f2) 0.0f; acc[ 1 ] = (f2) 0.0f; acc[ 2 ] = (f2) 0.0f;

				df_load_at< KH, NPH, BI, 0 >( d0, ad );
				df_load_at< KH, NPH, BI, BI >( d1, ad );
				df_wait< BI, BI >( d0 );
				df_feed_batch< KH, NTH, BI, 0 >( acc, d0, cp );
				df_load_at< KH, NPH, BI, 2 * BI >( d2, ad );
				df_wait< BI, BI >( d1 );
				df_feed_batch< KH, NTH, BI, BI >( acc, d1, cp );
				df_load_at< KH, NPH, BI, 3 * BI >( d3, ad );
				df_wait< BI, BI >( d2 );
				df_feed_batch< KH, NTH, BI, 2 * BI >( acc, d2, cp );
				df_wait< BI, 0 >( d3 );
				df_feed_batch< KH, NTH, BI, 3 * BI >( acc, d3, cp );

				f2* tp = (f2*) &sT[ h ][ rho ][ 3 * tri ] + hf;
				tp[ 0 ] = acc[ 0 ];
				tp[ 2 ] = acc[ 1 ];
				tp[ 4 ] = acc[ 2 ];
			}

			// ---- T values outside the array are copies of the edge values
			// (the reference replicates the resize OUTPUT, avir.h:3227-3239)
			if( edge )
			{
				if( lane < DF_NT1 )
				{
					const int x = X0 + lane;

					if( x < 0 || x > olast )
					{
						const int xs = dn_clampi( x, olast ) - X0;
						const f4 v0 = sT[ h ][ 0 ][ xs ];
						const f4 v1 = sT[ h ][ 1 ][ xs ];
						sT[ h ][ 0 ][ lane ] = v0;
						sT[ h ][ 1 ][ lane ] = v1;
					}
				}
			}

			// ---- correction FIR along x: 2 rows x 42 pixels x 2 halves
			if( !( dbg & 8 ))
#pragma unroll
			for( int q = 0; q < 3; q++ )
			{
				const int task = q * 64 + lane;

				if( task < 2 * DF_W * 2 )
				{
					const int r2 = ( task >= DF_W * 2 ? 1 : 0 );
					const int pp = task - r2 * DF_W * 2;
					const f2* t = (const f2*) &sT[ h ][ r2 ][ 0 ] + pp;
					f2 a = f0 * t[ 6 ];
					a = a + f1 * ( t[ 8 ] + t[ 4 ]);
					a = a + f2_ * ( t[ 10 ] + t[ 2 ]);
					a = a + f3 * ( t[ 12 ] + t[ 0 ]);
					*( (f2*) &sF[ bf ][ 2 * h + r2 ][ 0 ] + pp ) = a;
				}
			}

			DF_TIMED( tk_bar, __syncthreads());
		}
	}
	else
	{
		// ------------------------------------------------------------
		// column waves
		// ------------------------------------------------------------
		// (Raising the column waves' priority, s_setprio 3, moves the barrier
		// wait from the row waves -- 28 % of their time at equal priority,
		// in-kernel clocks of AVIRHIP_DNF_DBG=16 -- to the column waves, 47 %,
		// and the launch takes as long: the step is bound by the SIMDs' total
		// issue, not by one role. Skewing the row waves of a SIMD against each
		// other with s_sleep costs 3-5 %.)
		// K = 2 along y: the column waves are the step's longest instruction
		// streams (12 taps and a correction-filter row every second source
		// row) and the row waves spend 40 % of their time in the barrier;
		// raised, a column wave issues whenever it can (3840x2160 ->
		// 1920x1080: 0.0636 -> 0.0615 ms)
		if( KV == 2 )
		{
			__builtin_amdgcn_s_setprio( 3 );
		}

		const int vi = wave - DF_NHW;
		const bool lane_ok = ( lane < DF_LPV );
		const int e = DF_LPV * vi + ( lane_ok ? lane : DF_LPV - 1 );
		const int x = strip * DF_W + ( e >> 2 );
		const int ch = e & 3;
		const bool st_ok = ( lane_ok && x < P.H.out_len );

		// the tap pairs (see DF_VSTMT): one copy per lane, in registers
		f2 k2[ NTV + 2 * KV ];
		{
			const f2* const v2 = (const f2*) ( P.V.coef + NTV + 4 );
#pragma unroll
			for( int i = 0; i < NTV + 2 * KV; i++ )
			{
				k2[ i ] = v2[ i ];
			}
#pragma unroll
			for( int i = 0; i < NTV + 2 * KV; i++ )
			{
				asm volatile( "" : "+v"( k2[ i ])); // (no re-loading later)
			}
		}

		gp_cfloat* const vc = (gp_cfloat*) P.V.coef;
		const float f0 = vc[ NTV ], f1 = vc[ NTV + 1 ], f2_ = vc[ NTV + 2 ],
			f3 = vc[ NTV + 3 ];

		// destination: lane offset fixed, row offset scalar; lanes that must
		// not store get an offset the buffer range check drops
		int st_voff;
		__amdgpu_buffer_rsrc_t drs;

		if( P.out.on != 0 )
		{
			const int es = ( OUT == DH_S8 ? 1 : OUT != DH_F32 ? 2 :
				P.out.type == AVIRHIP_U8 ? 1 :
				( P.out.type == AVIRHIP_U16 ? 2 : 4 ));

			drs = __builtin_amdgcn_make_buffer_rsrc( P.out.base, 0,
				0x7fffffff, 0x00020000 );
			st_voff = ( st_ok && ch < P.out.ch ?
				( x * P.out.ch + ch ) * es : (int) 0x80000000 );
		}
		else
		{
			drs = __builtin_amdgcn_make_buffer_rsrc( (void*) P.dst, 0,
				0x7fffffff, 0x00020000 );
			st_voff = ( st_ok ? ( x * 4 + ch ) * 4 : (int) 0x80000000 );
		}

		f2 accp[ 8 ];
		float wr[ 8 ];
#pragma unroll
		for( int i = 0; i < 8; i++ )
		{
			accp[ i ] = (f2) 0.0f;
			wr[ i ] = 0.0f;
		}

		// a uint8 result under gamma: the step's outputs (one every KV rows)
		// wait here for the searches and stores at the end of the step; the
		// thresholds of the lane's channel (the colour or the alpha half)
		constexpr int NGO = DF_RS / KV;
		float gv[ NGO ];
		int gyr[ NGO ];
		bool g_alpha = false;
		const float* gthr = nullptr;

		if constexpr( S8 )
		{
			dh_fill_tables< SRC, OUT >( PA.G, tid );
			__syncthreads();
		}

		if constexpr( OUT == DH_S8 )
		{
			g_alpha = ( ch == PA.G.alpha_index );
			gthr = ds_table< 512 >() + ( g_alpha ? 256 : 0 );
		}

		int s = 0;
		int jl_base = 0; // local index of the output in slot 0 of this period

		while( s < S )
		{
			dn_static_for< DF_NPH >( [&]( auto phc )
			{
				constexpr int ph = decltype( phc )::value;

				if( s < S )
				{
					DF_TIMED( tk_bar, __syncthreads());

					if constexpr( OUT == DH_S8 )
					{
#pragma unroll
						for( int k = 0; k < NGO; k++ )
						{
							gv[ k ] = 0.0f;
							gyr[ k ] = -1;
						}
					}
					f2 vp[ DF_RS / 2 ];
#pragma unroll
					for( int m = 0; m < DF_RS / 2; m++ )
					{
						vp[ m ].x = sF[ s & 1 ][ 2 * m ][ e ];
						vp[ m ].y = sF[ s & 1 ][ 2 * m + 1 ][ e ];
					}

					if( !( dbg & 1 ))
					dn_static_for< DF_RS >( [&]( auto ic )
					{
						constexpr int i = decltype( ic )::value;
						constexpr int u = ph * DF_RS + i; // row of the period
						constexpr DfRow< KV, NTV, u > R;

						// the sum of an output starts from +0.0f
						if constexpr( R.zslot >= 0 )
						{
							constexpr int zp = ( R.zslot >> 2 ) * 2 +
								( R.zslot & 1 );

							if constexpr((( R.zslot >> 1 ) & 1 ) == 0 )
							{
								accp[ zp ].x = 0.0f;
							}
							else
							{
								accp[ zp ].y = 0.0f;
							}
						}

#define DF_PI( k ) accp[ R.pi[ ( k ) < R.n ? ( k ) : 0 ]]
#define DF_KI( k ) k2[ R.vi[ ( k ) < R.n ? ( k ) : 0 ]]
						df_vstmt< R.n, ( i & 1 ) >( DF_PI( 0 ), DF_PI( 1 ),
							DF_PI( 2 ), DF_PI( 3 ), DF_PI( 4 ), DF_PI( 5 ),
							DF_PI( 6 ), DF_PI( 7 ), vp[ i >> 1 ], DF_KI( 0 ),
							DF_KI( 1 ), DF_KI( 2 ), DF_KI( 3 ), DF_KI( 4 ),
							DF_KI( 5 ), DF_KI( 6 ), DF_KI( 7 ));
#undef DF_PI
#undef DF_KI

						// a T row completes with its last tap
						if constexpr(( u - ( NTV - 1 )) % KV == 0 )
						{
							constexpr int jp = ( u - ( NTV - 1 )) / KV;
							constexpr int slot = (( jp % 16 ) + 16 ) % 16;
							constexpr int sp = ( slot >> 2 ) * 2 + ( slot & 1 );
							constexpr int ws = (( jp % 8 ) + 8 ) % 8;
							const int jl = jl_base + jp;

							if( jl >= 0 )
							{
								const int j = jstart + jl;
								float U = ((( slot >> 1 ) & 1 ) == 0 ?
									accp[ sp ].x : accp[ sp ].y );

								if( j > vlast )
								{
									U = wr[ ( ws + 7 ) & 7 ];
								}

								if( jl == 0 && top )
								{
#pragma unroll
									for( int k = 0; k < 8; k++ )
									{
										wr[ k ] = U;
									}
								}

								wr[ ws ] = U;
								const int y = j - 3;

								if( y >= oy0 && y < oy1 )
								{
									float a = f0 * wr[ ( ws + 5 ) & 7 ];
									a = a + f1 * ( wr[ ( ws + 6 ) & 7 ] +
										wr[ ( ws + 4 ) & 7 ]);
									a = a + f2_ * ( wr[ ( ws + 7 ) & 7 ] +
										wr[ ( ws + 3 ) & 7 ]);
									a = a + f3 * ( wr[ ws ] +
										wr[ ( ws + 2 ) & 7 ]);

									const int yr = y - P.dst_row0;

									if constexpr( OUT == DH_S8 )
									{
										// (outputs complete every KV rows:
										// the step's i / KV-th)
										gv[ i / KV ] = a;
										gyr[ i / KV ] = yr;
									}
									else
									if constexpr( OUT != DH_F32 )
									{
										__builtin_amdgcn_raw_buffer_store_b16(
											dh_narrow< OUT >( a ), drs, st_voff,
											yr * (int) P.out.stride * 2, 0 );
									}
									else
									if( P.out.on == 0 )
									{
										__builtin_amdgcn_raw_buffer_store_b32(
											__builtin_bit_cast( unsigned, a ),
											drs, st_voff,
											yr * (int) P.dst_ss * 4, 0 );
									}
									else
									{
										df_store_elem( P.out, drs, st_voff, yr,
											a );
									}
								}
							}
						}
					} );

					if constexpr( OUT == DH_S8 )
					{
						int lo[ NGO ];
						dh_count< NGO >( lo, gv, gthr );

						// outside the range the thresholds were searched in the
						// direct expression decides (dnsrgb_dev.h). Nothing an
						// image holds: ONE copy of it per step, a loop over
						// the lane's such values
						unsigned int far = 0u;
#pragma unroll
						for( int k = 0; k < NGO; k++ )
						{
							far |= ( !( fabsf( gv[ k ]) <= 16.0f ) ? 1u << k :
								0u );
						}

#pragma nounroll
						while( far != 0u )
						{
							const int kf = __builtin_ctz( far );
							far &= far - 1u;
							float v = gv[ 0 ];
#pragma unroll
							for( int k = 1; k < NGO; k++ )
							{
								v = ( kf == k ? gv[ k ] : v );
							}

							const int bt = ds_direct_byte( v, g_alpha, PA.G );
#pragma unroll
							for( int k = 0; k < NGO; k++ )
							{
								lo[ k ] = ( kf == k ? bt : lo[ k ]);
							}
						}

#pragma unroll
						for( int k = 0; k < NGO; k++ )
						{
							if( gyr[ k ] >= 0 )
							{
								__builtin_amdgcn_raw_buffer_store_b8(
									(unsigned char) lo[ k ], drs, st_voff,
									gyr[ k ] * (int) P.out.stride, 0 );
							}
						}
					}

					s++;
				}
			} );

			jl_base += DF_NPH * DF_RS / KV;
		}
	}

	if(( dbg & 16 ) && lane == 0 && P.clk != nullptr )
	{
		unsigned long long* const q = P.clk + ( (size_t) item * 12 + wave ) * 4;
		q[ 0 ] = __builtin_readcyclecounter() - tk_total;
		q[ 1 ] = tk_dma; q[ 2 ] = tk_bar; q[ 3 ] = (unsigned long long) S;
	}
}

// float RGBA rows on both sides, with the ablations and the clocks
template< int KH, int NTH, int KV, int NTV, int DF_NHW >
__global__ void __launch_bounds__( DF_NTHR ) k_dnf( const DnFParams P )
{
	df_march< KH, NTH, KV, NTV, DF_NHW, DH_F32, DH_F32, true >( P );
}

// every other pair of kinds
template< int KH, int NTH, int KV, int NTV, int DF_NHW, int SRC, int OUT >
__global__ void __launch_bounds__( DF_NTHR ) k_dnfh(
	const typename DhParams< SRC, OUT >::type PA )
{
	static_assert( SRC != DH_F32 || OUT != DH_F32, "float -> float is k_dnf" );
	constexpr bool S8 = ( SRC == DH_S8 || OUT == DH_S8 );
	static_assert( !S8 || (( SRC == DH_S8 || SRC == DH_F32 ) &&
		( OUT == DH_S8 || OUT == DH_F32 )), "gamma: uint8 and float sides" );
	df_march< KH, NTH, KV, NTV, DF_NHW, SRC, OUT, false >( PA );
}

// ---------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------

static DnAxisP dnf_axis( const DnAxis& A )
{
	DnAxisP P;
	P.K = A.K; P.NT = A.NT; P.c0 = A.c0;
	P.in_len = A.in_len; P.out_len = A.out_len; P.coef = A.d_coef;
	return( P );
}

// A launch's parameters: both axes of the plan, the source rows (`src_ss`
// elements of their type apart), destination rows [row0, row1), the output
// stage if there is one, and the chunk rule -- the grid is nstrips * nchunks
// work items. No ablations, no clocks.
static void dnf_fill( DnFParams& P, const DnData* D, const void* src,
	long src_ss, float* dst, int row0, int row1, const GPOut* out )
{
	P.H = dnf_axis( D -> h );
	P.V = dnf_axis( D -> v );
	P.src = (const float*) src; P.src_ss = src_ss;
	P.dst = dst; P.dst_ss = (long) D -> h.out_len * 4; P.dst_row0 = row0;
	P.row_lo = row0; P.row_hi = row1;
	memset( &P.out, 0, sizeof( P.out ));

	if( out != nullptr )
	{
		P.out = *out;
	}

	P.dbg = 0;
	P.clk = nullptr;
	P.nstrips = ( D -> h.out_len + DF_W - 1 ) / DF_W;
	const int rows = row1 - row0;
	P.crows = dnf_chunk_rows( rows, D -> ncu, P.nstrips );
	P.nchunks = ( rows + P.crows - 1 ) / P.crows;
}

// Both axes in one launch: float RGBA source rows -> destination rows
// [row0, row1) (row row0 at `dst`, or through the integer output stage `out`).
// Returns 1 when this call cannot take the fused kernel.
int dn_run_hv( void* d, const float* src, long src_ss, float* dst, int row0,
	int row1, hipStream_t st, const GPOut* out )
{
	const DnData* D = (const DnData*) d;

	if( D == nullptr || !D -> hok || !D -> vok )
	{
		return( 1 );
	}

	if( row1 <= row0 )
	{
		return( AVIRHIP_OK );
	}

	// (row offsets of the DMA are 32-bit)
	if( (long) D -> v.in_len * src_ss * 4 >= 0x7fffffffL )
	{
		return( 1 );
	}

	DnFParams P;
	dnf_fill( P, D, src, src_ss, dst, row0, row1, out );
	const dim3 grid( P.nstrips * P.nchunks );

	static const int dbg = []() { const char* e = getenv( "AVIRHIP_DNF_DBG" );
		return( e != nullptr ? atoi( e ) : 0 ); }();
	P.dbg = dbg;
	static unsigned long long* dclk = nullptr;
	static int dcalls = 0;

	// (debugging aid, single-threaded use: per-wave clocks of up to 4096 work
	// items; larger launches and a failed allocation run without them)
	if(( dbg & 16 ) && grid.x <= 4096 )
	{
		if( dclk == nullptr && hipMalloc( &dclk, 4096 * 12 * 32 ) != hipSuccess )
		{
			(void) hipGetLastError();
			dclk = nullptr;
		}

		P.clk = dclk;
	}
	const int kk = D -> h.K * 10 + D -> v.K;
	// K = 3 along y: 9 row waves + 3 column waves (AVIRHIP_DNF_NHW=8: the 8 + 4
	// split, for A/B timing)
	static const int nhw3 = []() { const char* e = getenv( "AVIRHIP_DNF_NHW" );
		return( e != nullptr && atoi( e ) == 8 ? 8 : 9 ); }();

#define DF_LAUNCH( ... ) hipLaunchKernelGGL(( k_dnf< __VA_ARGS__ > ), grid, \
	dim3( DF_NTHR ), 0, st, P )

	switch( kk )
	{
		case 33:
			if( nhw3 == 9 ) DF_LAUNCH( 3, 38, 3, 38, 9 );
			else DF_LAUNCH( 3, 38, 3, 38, 8 );
			break;
		case 22:
			DF_LAUNCH( 2, 24, 2, 24, 8 );
			break;
		case 32:
			DF_LAUNCH( 3, 38, 2, 24, 8 );
			break;
		case 23:
			if( nhw3 == 9 ) DF_LAUNCH( 2, 24, 3, 38, 9 );
			else DF_LAUNCH( 2, 24, 3, 38, 8 );
			break;
		default:
			return( 1 );
	}

#undef DF_LAUNCH
	dnf_verbose( "k_dnf", P.nstrips, P.nchunks, P.crows );

	if(( dbg & 16 ) && P.clk != nullptr && ++dcalls == 100 )
	{
		// in-kernel clocks of a launch in the middle of a timing loop
		std::vector< unsigned long long > hc( (size_t) grid.x * 12 * 4 );
		(void) hipStreamSynchronize( st );
		(void) hipMemcpy( hc.data(), dclk, hc.size() * 8, hipMemcpyDeviceToHost );
		const int nh = ( D -> v.K == 3 ? nhw3 : 8 );
		double tot[ 2 ] = { 0, 0 }, dma[ 2 ] = { 0, 0 }, bar[ 2 ] = { 0, 0 };
		double mx = 0.0;

		for( unsigned i = 0; i < grid.x; i++ )
		{
			for( int wv = 0; wv < 12; wv++ )
			{
				const unsigned long long* q = &hc[ ( (size_t) i * 12 + wv ) * 4 ];
				const int r = ( wv < nh ? 0 : 1 );
				tot[ r ] += (double) q[ 0 ]; dma[ r ] += (double) q[ 1 ];
				bar[ r ] += (double) q[ 2 ];
				mx = std::max( mx, (double) q[ 0 ]);
			}
		}

		const double nr = (double) grid.x * nh, nc = (double) grid.x * ( 12 - nh );
		fprintf( stderr, "k_dnf clocks (%u items, %d row waves): row waves total "
			"%.0f, DMA wait %.0f, barrier %.0f | column waves total %.0f, "
			"barrier %.0f | longest wave %.0f cycles, %llu steps\n", grid.x, nh,
			tot[ 0 ] / nr, dma[ 0 ] / nr, bar[ 0 ] / nr, tot[ 1 ] / nc,
			bar[ 1 ] / nc, mx, hc[ 3 ]);
	}
	AVIRHIP_HIPCHECK( hipGetLastError() );
	return( AVIRHIP_OK );
}

static int dh_kind( const int type )
{
	return( type == AVIRHIP_F16 ? DH_F16 :
		( type == AVIRHIP_BF16 ? DH_BF16 : DH_F32 ));
}

// The launcher of k_dnfh: RGBA source rows of `src`, read where they lie ->
// destination rows [row0, row1): float RGBA rows at `dst` (out == nullptr), or
// through `out`.
//   G == nullptr  half, bfloat16 or float rows; half / bfloat16 elements
//                 narrowed in the store, or the integer output stage
//   G != nullptr  sRGB gamma: uint8 or float rows (the pack pass's linear copy);
//                 a uint8 result of 1-4 channels de-linearised and stored
//                 bytewise, or float rows (linear)
// Returns 1 when the call is not this kernel's: float on both sides (k_dnf's),
// a 16-bit image lanc2h_image_ok refuses, a uint8 source whose base or pitch is
// no multiple of 4 bytes, rows beyond a 32-bit byte offset.
static int dh_run( void* d, const ImageRef& src, float* dst, int row0, int row1,
	hipStream_t st, const GPOut* out, const DnGamma* G )
{
	const DnData* D = (const DnData*) d;
	int sk, ok;

	if( G != nullptr )
	{
		sk = ( src.type == AVIRHIP_U8 ? DH_S8 : DH_F32 );
		ok = ( out != nullptr ? DH_S8 : DH_F32 );

		if(( sk == DH_F32 && src.type != AVIRHIP_F32 ) ||
			( out != nullptr && ( out -> type != AVIRHIP_U8 || out -> ch < 1 ||
			out -> ch > 4 || G -> thr == nullptr )) ||
			( sk == DH_S8 && ( G -> tbl == nullptr ||
			( (uintptr_t) src.ptr & 3 ) != 0 || ( src.stride & 3 ) != 0 )) ||
			( sk == DH_F32 && (( (uintptr_t) src.ptr & 15 ) != 0 ||
			( src.stride & 3 ) != 0 )))
		{
			return( 1 );
		}
	}
	else
	{
		sk = dh_kind( src.type );
		ok = ( out != nullptr ? dh_kind( out -> type ) : DH_F32 );

		if( !lanc2h_image_ok( src.ptr, src.type, src.stride ) ||
			( ok != DH_F32 && ( (uintptr_t) out -> base & 1 ) != 0 ))
		{
			return( 1 );
		}
	}

	if( D == nullptr || !D -> hok || !D -> vok || src.ch != 4 ||
		( sk == DH_F32 && ok == DH_F32 ) ||
		( out == nullptr && ( dst == nullptr || ( (uintptr_t) dst & 15 ) != 0 )))
	{
		return( 1 );
	}

	if( row1 <= row0 )
	{
		return( AVIRHIP_OK );
	}

	// (row offsets of the loads and of the 8- and 16-bit stores are 32-bit, in
	// bytes)
	const long spb = src.stride * ( sk == DH_F32 ? 4L : ( sk == DH_S8 ? 1L :
		2L ));

	if( (long) D -> v.in_len * spb >= 0x7fffffffL ||
		( ok != DH_F32 && (long) ( row1 - row0 ) * out -> stride *
		( ok == DH_S8 ? 1 : 2 ) >= 0x7fffffffL ))
	{
		return( 1 );
	}

	DnSParams PS;
	DnFParams& P = PS.F;
	dnf_fill( P, D, src.ptr, src.stride, dst, row0, row1, out );
	const dim3 grid( P.nstrips * P.nchunks );
	memset( &PS.G, 0, sizeof( PS.G ));

	if( G != nullptr )
	{
		PS.G = *G;
	}

#define DH_LAUNCH( SK, OK ) hipLaunchKernelGGL(( k_dnfh< KH, NTH, KV, NTV, NHW, \
	SK, OK > ), grid, dim3( DF_NTHR ), 0, st, P )
#define DH_LAUNCH8( SK, OK ) hipLaunchKernelGGL(( k_dnfh< KH, NTH, KV, NTV, NHW, \
	SK, OK > ), grid, dim3( DF_NTHR ), 0, st, PS )
#define DH_FORM( KH_, NTH_, KV_, NTV_, NHW_ ) do { \
	constexpr int KH = KH_, NTH = NTH_, KV = KV_, NTV = NTV_, NHW = NHW_; \
	switch( sk * 4 + ok ) \
	{ \
		case DH_F32 * 4 + DH_F16: DH_LAUNCH( DH_F32, DH_F16 ); break; \
		case DH_F32 * 4 + DH_BF16: DH_LAUNCH( DH_F32, DH_BF16 ); break; \
		case DH_F16 * 4 + DH_F32: DH_LAUNCH( DH_F16, DH_F32 ); break; \
		case DH_F16 * 4 + DH_F16: DH_LAUNCH( DH_F16, DH_F16 ); break; \
		case DH_F16 * 4 + DH_BF16: DH_LAUNCH( DH_F16, DH_BF16 ); break; \
		case DH_BF16 * 4 + DH_F32: DH_LAUNCH( DH_BF16, DH_F32 ); break; \
		case DH_BF16 * 4 + DH_F16: DH_LAUNCH( DH_BF16, DH_F16 ); break; \
		case DH_BF16 * 4 + DH_BF16: DH_LAUNCH( DH_BF16, DH_BF16 ); break; \
		case DH_S8 * 4 + DH_S8: DH_LAUNCH8( DH_S8, DH_S8 ); break; \
		case DH_S8 * 4 + DH_F32: DH_LAUNCH8( DH_S8, DH_F32 ); break; \
		case DH_F32 * 4 + DH_S8: DH_LAUNCH8( DH_F32, DH_S8 ); break; \
		default: return( 1 ); \
	} } while( 0 )

	// (K = 3 along y: the 9 + 3 split, k_dnf's default)
	switch( D -> h.K * 10 + D -> v.K )
	{
		case 33: DH_FORM( 3, 38, 3, 38, 9 ); break;
		case 22: DH_FORM( 2, 24, 2, 24, 8 ); break;
		case 32: DH_FORM( 3, 38, 2, 24, 8 ); break;
		case 23: DH_FORM( 2, 24, 3, 38, 9 ); break;
		default: return( 1 );
	}

#undef DH_FORM
#undef DH_LAUNCH8
#undef DH_LAUNCH
	dnf_verbose( "k_dnfh", P.nstrips, P.nchunks, P.crows );

	AVIRHIP_HIPCHECK( hipGetLastError() );
	return( AVIRHIP_OK );
}

// dn_run_hv with half / bfloat16 pixels on a side
int dn_run_hv16( void* d, const ImageRef& src, float* dst, int row0, int row1,
	hipStream_t st, const GPOut* out )
{
	return( dh_run( d, src, dst, row0, row1, st, out, nullptr ));
}

// ... with sRGB gamma and 8-bit pixels on a side
int dn_run_hv8( void* d, const ImageRef& src, float* dst, int row0, int row1,
	hipStream_t st, const GPOut* out, const DnGamma& G )
{
	return( dh_run( d, src, dst, row0, row1, st, out, &G ));
}

} // namespace avirhip
