// up2.hip -- the headline kernel: exact 2x RGBA upsizing (cfg2/cfg3 of
// BASELINE.json), H pass + V pass fused in ONE launch.
//
// What the plan looks like (default parameters, mode 1 or 3), per
// axis with source length W:
//   C[m]  = f0*S[m-3] + sum_{i=1..3} f_i*(S[m-3+i] + S[m-3-i])     (7-tap FIR,
//           EdgePixelCount 3; doFilter avir.h:3748)
//   up    = zero-stuffed 2x view of C                   (doUpsample, 3260-3402)
//   o[2q]   = 0 + sum_{t<12} Fe[t]*C[q-3+t]             (doResize2, 4114-4328:
//   o[2q+1] = 0 + sum_{t<12} Fo[t]*C[q-2+t]              one bank phase, x = 0)
// with every index clamped to the producing array's range. Because edge
// replication makes Sext[u] = S[clamp(u)] constant outside the image, the
// clamped C equals FIR(Sext[m-6..m]) for EVERY m -- so no border special
// cases exist anywhere below, only clamped source loads.
//
// Structure ("marching strip"): a workgroup (2 waves) owns a strip of 64 output
// columns and a chunk of output rows, and marches down the source U2_RB rows
// at a time, two barriers per step:
//   S   U2_RB source rows x 50 px (halo 9+9): HBM -> LDS by LDS-DMA
//       (buffer_load_dwordx4 ... lds), no staging registers
//   H1  C rows  = FIR7 along x, whole pixels                     LDS -> LDS
//   H2  T rows  = 12-tap even/odd interpolation along x (a thread streams
//       once over a row's C half pixels and feeds the 8 sums of four source
//       pixels U2_HS apart: a tap product shared by an even and an odd sum
//       is multiplied once -- see h2_phase)                      LDS -> LDS
//   V   each thread owns ONE HALF-PIXEL output column (8 bytes) and keeps the
//       vertical FIR window (7) and the vertical interpolation window (13) in
//       REGISTERS, rotating through statically-indexed ring slots (the 16-row
//       ring period is fully unrolled), consuming one T row per step from LDS
//       and streaming two output rows per step straight to HBM (nt stores,
//       512 contiguous bytes per wave-instruction).
// Pipeline: interval B = {DMA of the next S tile in flight, H2 of this step};
// interval A = {V of this step with H1 of the NEXT step woven into it}.
// The horizontally resized intermediate (the reference's FltBuf) never exists
// in memory, vertical work is never recomputed inside a chunk, and all 56
// filter coefficients are wave-uniform scalar operands (Taps).
//
// Arithmetic contract: -ffp-contract=off, mul then add in the reference's tap
// order, interpolation sums started from +0.0f => bit-identical output.

#include "plan.h"
#include "up2_chunks.h"
#include "up2_params.h"
#include <algorithm>
#include <string.h>
#include <stdlib.h>
#include <stdio.h>
#include <type_traits>

namespace avirhip {

typedef float f4 __attribute__(( ext_vector_type( 4 )));
typedef float f2 __attribute__(( ext_vector_type( 2 )));
typedef unsigned u2 __attribute__(( ext_vector_type( 2 )));

#ifndef U2_TW
#define U2_TW 64 // output columns per strip (32: one autonomous wave per strip)
#endif
#define U2_NT ( U2_TW * 2 ) // threads per workgroup: one per half pixel
#ifndef U2_RB
#define U2_RB 8   // source rows per marching step (8 or 16)
#endif
#ifndef U2_HS
#define U2_HS 4   // H2 (transposed form): distance of a thread's four source pixels (2 or 4)
#endif
#define U2_SW ( U2_TW / 2 + 18 ) // S tile width (px)
#define U2_CW ( U2_TW / 2 + 12 ) // C tile width (px)

// (Up2Params, the kernel's parameters, and Up2GParams, which the sRGB gamma
// kinds take instead: up2_params.h. tests/align_cases.py, tests/far_row_cases.py
// and DESIGN's alignment tables quote lines of this file by number.)

// The 28 wave-uniform filter taps of one axis, in two layouts (up2_prepare):
//   packed (the transposed form, k_up2< true >): ONE float per tap,
//       [f 4 | fe 12 | fo 12 | pad 4] per axis at coef + 0 / + 32. A tap enters
//       v_pk_mul_f32 as the 64-bit scalar operand of the aligned SGPR pair it
//       lies in, broadcast to both halves by op_sel / op_sel_hi (the compiler
//       folds splat() below into them; for some odd taps it copies the tap
//       into the low half of a pair of its own with one s_mov) -- half the
//       SGPRs of the paired layout, which filled the SGPR file of this form
//       and spilled 58 SGPRs into VGPR lanes (v_readlane in the marching loop).
//   paired (the plain form, k_up2< false >): every tap an aligned pair {c, c},
//       [f 4x2 | fe 12x2 | fo 12x2 | pad 8] per axis at coef + U2_PAIRED /
//       + U2_PAIRED + 64. Its vertical phase reads all 28 vertical taps in
//       every row; from the packed layout the compiler's s_mov copies of the
//       odd ones cost more SGPRs than the pairs (spills 19 -> 53).
// They are loaded per phase with a volatile scalar load: letting the compiler
// hoist both axes' taps out of the marching loop overflowed the SGPR file.
typedef float f8 __attribute__(( ext_vector_type( 8 )));
typedef float f16 __attribute__(( ext_vector_type( 16 )));
#define U2_PAIRED 64 // floats: the paired layout's offset in Up2Params::coef

// (wave-uniform tap) -> the packed operand {c, c}
__device__ __forceinline__ f2 splat( const float c )
{
	f2 r; r.x = c; r.y = c; return( r );
}

// the whole axis, paired (the plain form)
struct Taps
{
	f16 a, b, c; // f0..3 fe0..3 | fe4..11 | fo0..7   (as pairs)
	f8 d;        // fo8..11
	__device__ __forceinline__ f2 pr( const f16& v, int i ) const
		{ f2 r; r.x = v[ 2 * i ]; r.y = v[ 2 * i + 1 ]; return( r ); }
	__device__ __forceinline__ f2 f( int i ) const { return( pr( a, i )); }
	__device__ __forceinline__ f2 fe( int i ) const
		{ return( i < 4 ? pr( a, 4 + i ) : pr( b, i - 4 )); }
	__device__ __forceinline__ f2 fo( int i ) const
	{
		if( i < 8 ) return( pr( c, i ));
		f2 r; r.x = d[ 2 * ( i - 8 )]; r.y = d[ 2 * ( i - 8 ) + 1 ];
		return( r );
	}
};

// (forces a wave-uniform pointer into an SGPR pair: under register pressure
// the compiler may otherwise hand the asm a VGPR pair)
__device__ __forceinline__ const float* sgpr_ptr( const float* p )
{
	const unsigned long long a = (unsigned long long) p;
	const unsigned lo = __builtin_amdgcn_readfirstlane( (unsigned) a );
	const unsigned hi = __builtin_amdgcn_readfirstlane( (unsigned) ( a >> 32 ));
	return( (const float*) (( (unsigned long long) hi << 32 ) | lo ));
}

__device__ __forceinline__ Taps load_taps( const float* p0 )
{
	const float* const p = sgpr_ptr( p0 );
	Taps t;
	asm volatile( "s_load_dwordx16 %0, %4, 0x0\n\t"
		"s_load_dwordx16 %1, %4, 0x40\n\t"
		"s_load_dwordx16 %2, %4, 0x80\n\t"
		"s_load_dwordx8 %3, %4, 0xc0\n\t"
		AVIRHIP_WAITCNT_LGKM( 0 )
		: "=&s"( t.a ), "=&s"( t.b ), "=&s"( t.c ), "=&s"( t.d )
		: "s"( p ) : "memory" );
	return( t );
}

// packed fe0..11 (the horizontal interpolation: a bit-symmetric bank phase,
// fo[t] == fe[11-t], needs no fo -- 12 SGPRs)
struct TapsI
{
	f8 a; // fe0..7
	f4 b; // fe8..11
	__device__ __forceinline__ f2 fe( int i ) const
		{ return( splat( i < 8 ? a[ i ] : b[ i - 8 ])); }
};

__device__ __forceinline__ TapsI load_taps_i( const float* p0 )
{
	const float* const p = sgpr_ptr( p0 );
	TapsI t;
	asm volatile( "s_load_dwordx8 %0, %2, 0x10\n\t"
		"s_load_dwordx4 %1, %2, 0x30\n\t"
		AVIRHIP_WAITCNT_LGKM( 0 )
		: "=&s"( t.a ), "=&s"( t.b ) : "s"( p ) : "memory" );
	return( t );
}

// packed f0..3 and fe0..11 (the transposed vertical phase needs no fo)
struct TapsE
{
	f16 a;
	__device__ __forceinline__ f2 f( int i ) const { return( splat( a[ i ])); }
	__device__ __forceinline__ f2 fe( int i ) const { return( splat( a[ 4 + i ])); }
};

__device__ __forceinline__ TapsE load_taps_e( const float* p0 )
{
	const float* const p = sgpr_ptr( p0 );
	TapsE t;
	asm volatile( "s_load_dwordx16 %0, %1, 0x0\n\t"
		AVIRHIP_WAITCNT_LGKM( 0 )
		: "=&s"( t.a ) : "s"( p ) : "memory" );
	return( t );
}

// packed f0..3 (the horizontal FIR)
__device__ __forceinline__ f4 load_f4( const float* p0 )
{
	const float* const p = sgpr_ptr( p0 );
	f4 t;
	asm volatile( "s_load_dwordx4 %0, %1, 0x0\n\t" AVIRHIP_WAITCNT_LGKM( 0 )
		: "=&s"( t ) : "s"( p ) : "memory" );
	return( t );
}

// paired f0..3 (the horizontal FIR of the plain form)
__device__ __forceinline__ f8 load_f8( const float* p0 )
{
	const float* const p = sgpr_ptr( p0 );
	f8 t;
	asm volatile( "s_load_dwordx8 %0, %1, 0x0\n\t" AVIRHIP_WAITCNT_LGKM( 0 )
		: "=&s"( t ) : "s"( p ) : "memory" );
	return( t );
}

// (wave-uniform tap pair) * (whole pixel) = two v_pk_mul_f32
__device__ __forceinline__ f4 tmul( const f2 t, const f4 v )
{
	const f2 lo = t * v.lo;
	const f2 hi = t * v.hi;
	return( __builtin_shufflevector( lo, hi, 0, 1, 2, 3 ));
}

// The thread index, recomputed from the lane id: per-lane addresses derived
// from it inside a phase need no registers while the other phases run (the
// compiler cannot see through the asm, so it cannot keep them alive either).
__device__ __forceinline__ int fresh_tid( const int wave )
{
	int l;
	asm volatile( "v_mbcnt_lo_u32_b32 %0, -1, 0\n\t"
		"v_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"( l ));
	return( l + wave * 64 );
}

__device__ __forceinline__ int clampi( int i, int hi )
{
	return( i < 0 ? 0 : ( i > hi ? hi : i ));
}

// With one wave per workgroup no s_barrier is needed: LDS operations of a wave
// execute in program order, only the compiler must not reorder them.
#if U2_TW == 32
#define U2_SYNC() __builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" ); \
	__builtin_amdgcn_wave_barrier(); \
	__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" )
#else
// (the S tile's LDS-DMA is a compiler builtin: the compiler's own wait-count
// insertion drains it before the barrier; `make paranoid` drains by hand too)
#define U2_SYNC() do { AVIRHIP_BARRIER_DRAIN(); __syncthreads(); } while( 0 )

// Wave priority by interval (round 6, NOTEBOOK 10.11). The vertical interval
// -- 430 packed multiply-adds per lane and step, the result stores -- runs one
// step above the horizontal one (LDS window reads, the next tile's DMA): the
// four waves of a SIMD belong to workgroups in different intervals, and the
// arbiter's oldest-first choice otherwise lets a wave that is about to wait for
// LDS anyway take issue slots from the one whose arithmetic paces the step.
// Same-box, same-process: cfg3 -4.5 %, cfg2 -1.0 ... -1.5 %; any "vertical above
// horizontal" pair measures the same, the reverse +0.4 ... -1.2 %. Results do
// not depend on it.
#define U2_PRIO_H 0
#define U2_PRIO_V 1

// s_setprio takes an immediate
__device__ __forceinline__ void u2_setprio( const int p )
{
	if( p == 0 ) __builtin_amdgcn_s_setprio( 0 );
	else if( p == 1 ) __builtin_amdgcn_s_setprio( 1 );
	else if( p == 2 ) __builtin_amdgcn_s_setprio( 2 );
	else __builtin_amdgcn_s_setprio( 3 );
}
#endif

#ifdef U2_DBG
#define U2_ON( bit ) ( !( P.dbg & ( bit )))
// Upper-bound ablations of the two levers VERDICT r5 #5 asks to be MEASURED
// (timing only: the results are wrong): bit 16 -- the third H1 iteration runs in
// wave 0 only, 2.5 iterations per wave and step instead of 3 (a 128-column
// strip's C tile is 608 px over 256 threads = 2.375: less H1 halo, and none of
// that build's costs -- 4-wave barriers, half the workgroups per CU); bit 32 --
// no horizontal phase at all in a chunk's last two marching steps (the T rows a
// chunk shares with the one below would come from an L2-resident scratch block
// instead of being recomputed: 16 of its 18 run-in rows, without the cost of
// writing and re-reading them).
#define U2_ABL_H1( k ) ( !( P.dbg & 16 ) || ( k ) < 2 || wave == 0 )
#define U2_ABL_TAIL() ( !( P.dbg & 32 ) || abl_tail == 0 )
#else
#define U2_ON( bit ) true
#define U2_ABL_H1( k ) true
#define U2_ABL_TAIL() true
#endif

#ifndef U2_STAUX
#define U2_STAUX 2 // destination stores are streaming: nt (measured -10 %)
#endif

#ifndef U2_LDAUX
#define U2_LDAUX 0 // cache policy of the source loads
#endif

#define U2_TPL ( U2_RB * ( U2_TW / 2 ) + 8 ) // px per T plane, incl. the 128-B skew

#ifndef U2_H2PB
#define U2_H2PB 4 // H2 (transposed form): stream positions per block of LDS reads
#endif

// VT ("vertical transposed"): when the bank phase is bit-symmetric (fo[t] ==
// fe[11-t], true for every parameter preset), the product fe[t]*C2[m] belongs to
// BOTH even(m+3-t) and odd(m-9+t). The vertical phase then keeps 24 running
// sums per thread instead of a 13-row window: each new C2 row costs 12
// multiplies + 24 adds instead of 24 + 24, every sum still receives its
// products in ascending tap order from a +0 start => same bits. The
// horizontal interpolation of this form shares products the same way
// (h2_phase), so it wants both axes' bank phases symmetric.
// IO (VT only): 0 the float RGBA result; 1 uint8, 2 uint16, 3 float pixels of
// P.ich channels stored by the vertical phase itself (a lane holds two
// channels of a pixel: one store per channel, lanes without one carry an
// out-of-range offset) -- no float result, no epilogue pass over it.
// 6: half RGBA pixels (AVIRHIP_F16: the float result narrowed nearest-even, no
// clamp -- a float-type source's sums are not known finite or small): a lane's
// two channels are adjacent, one dword store.
// 7: bfloat16 RGBA pixels (AVIRHIP_BF16) the same way: the two floats narrowed
// nearest-even (the (__bf16) cast: v_cvt_pk_bf16_f32 on gfx950), one dword.
// SRC (VT only): 0 float RGBA pixels by 16-byte LDS-DMA; 10 * element size +
// channels (13, 14, 23, 24: RGB / RGBA uint8 / uint16) the caller's integer
// image as it lies -- packScanline's (float) cast and zero padding
// (avir.h:2777-2840) without a float copy of the source: a lane DMAs the two
// aligned dwords that hold its pixel into the first bytes of the pixel's own
// region of the S tile, and -- the same lane, after its wave's DMA has landed,
// before the interval's closing barrier -- reads them back, converts and writes
// the float pixel in place. P.src then points at bytes, P.src_ss counts bytes.
// 100 + such a code (124: half RGBA): the elements are IEEE halves, widened
// exactly (v_cvt_f32_f16, denormals kept) instead of cast from integers.
// 200 + such a code (224: bfloat16 RGBA): the elements are upper halves of
// floats -- a shift and a mask per dword, no conversion.
// sRGB gamma (UseSRGBGamma) with 8-bit pixels, the stages of generic.hip's pack
// pass and output stage inside this launch (expressions: dnsrgb_dev.h; the
// parameters: Up2GParams):
// SRC 313 / 314: uint8 RGB / RGBA read as 13 / 14 are, linearised in land_raw --
// a colour channel is tbl[ byte ] from a workgroup LDS copy of the plan's
// 256-entry table, the alpha channel (float) byte * gm.
// IO 8: a uint8 result through the de-linearising stage: a channel's byte is the
// count of thresholds thr[ 1..255 ] <= v (k_epilogue_gamma_thr's eight compares
// over the colour or the alpha half of an LDS copy of the plan's 2 x 256
// thresholds); a value outside |v| <= 16 takes that kernel's direct branch.
// IO 9: the same behind a uint8 / uint16 source, without the direct branch (the
// bound: store_g). Their parameters: Up2GParams, and the kernel's own at
// the same kernel-argument offsets; the kinds without gamma are unchanged
// machine code.
// LDS: the 2 KB of thresholds leave seven workgroups a CU, with the 1 KB table
// of SRC 313 / 314 six (three waves a SIMD: what the attribute below says).
template< bool VT, int IO = 0, int SRC = 0 >
__global__ void __launch_bounds__( U2_NT ) __attribute__((
	amdgpu_waves_per_eu( SRC / 100 == 3 ? 3 : 4, 4 ))) k_up2( const Up2PT< IO > P )
{
	static_assert( IO == 0 || VT, "the fused output stage lives in the VT form" );
	static_assert( SRC == 0 || VT, "raw sources live in the VT form" );
	constexpr bool SHALF = ( SRC / 100 == 1 ); // raw elements are halves
	constexpr bool SBF16 = ( SRC / 100 == 2 ); // raw elements are bfloat16s
	constexpr int SESZ = ( SRC % 100 ) / 10; // bytes per source element (raw)
	constexpr int SCH = SRC % 10;        // channels of a source pixel (raw)
	static_assert( !( SHALF || SBF16 ) || SESZ == 2,
		"half / bfloat16 elements are two bytes" );
	constexpr int PXB = ( SRC != 0 ? SESZ * SCH : 16 ); // bytes per source pixel
	// (IO 4 / 5: uint8 / uint16 results of an INTEGER source -- finite and far
	// inside the int range, so the stage is add, convert, integer clamp)
	constexpr int ESZ = ( IO == 1 || IO == 4 || up2_gamma_out< IO > ? 1 :
		( IO == 2 || IO == 5 || IO == 6 || IO == 7 ? 2 : 4 ));
	// LDS tiles, whole pixels (16 B). The horizontal phases work on whole
	// pixels so that every LDS access is a conflict-free 128-bit one; the
	// vertical phase reads half pixels (8 B) of T.
	//   sS  U2_RB rows x U2_SW px, flat: exactly the lane order of the DMA
	//   sC  U2_RB rows x U2_CW px, flat
	//   sT  two planes (even / odd output column), U2_RB rows x U2_TW/2 px
	//       each; the planes sit 128 B (mod 256 B) apart so that the vertical
	//       phase's alternating-plane reads fall into disjoint banks
	__shared__ __attribute__(( aligned( 16 ))) f4 sS[ U2_RB * U2_SW ];
	__shared__ __attribute__(( aligned( 16 ))) f4 sC[ U2_RB * U2_CW ];
	__shared__ __attribute__(( aligned( 16 ))) f4 sT[ U2_TPL * 2 - 8 ];

#ifdef U2_DBG
	const unsigned long long dbg_c0 = clock64();
	const unsigned long long dbg_w0 = wall_clock64();

	// (bits 2048 / 4096: the workgroups of a CU start apart -- by half a
	// marching step in two groups, by eighths in eight -- instead of together)
	if( P.dbg & ( 2048 | 4096 ))
	{
		const int slot = ( P.dbg & 2048 ? (( blockIdx.x >> 8 ) & 1 ) * 4 :
			( blockIdx.x >> 8 ) & 7 );

		for( int i = 0; i < slot; i++ )
		{
			__builtin_amdgcn_s_sleep( 25 ); // 1,600 cycles: an eighth of a step
		}
	}
#endif
	// XCD-aware dealing of (strip, chunk) work items (see fused.hip)
	const int nwg = gridDim.x;
	const int b = blockIdx.x;
	const int xcd = b & 7;
	const int qd = nwg >> 3;
	const int rm = nwg & 7;
	const int item = ( xcd < rm ? xcd * ( qd + 1 ) :
		rm * ( qd + 1 ) + ( xcd - rm ) * qd ) + ( b >> 3 );

	// strip-major: an XCD's contiguous item range holds whole strips, i.e.
	// the same mix of long and short chunks as every other XCD; a strip's
	// long chunks come first
	const int strip = item / P.nchunks;
	const int chunk = P.chunk0 + item - strip * P.nchunks;
	const int tid = threadIdx.x;
	const int hf = tid & 1;   // which half of the pixel (channels 0-1 / 2-3)
	const int col = tid >> 1; // column within the strip (vertical phase)

	const int qx0 = strip * ( U2_TW / 2 );
	const int qy0 = up2_chunk_first( chunk, P.cq, P.nlong );
	const int qy1 = min( qy0 + up2_chunk_rows( chunk, P.cq, P.nlong ),
		P.nh >> 1 );
	const int u0 = qy0 - 9;               // first Text row index consumed
	const int nsteps = qy1 - qy0 + 18;    // 6 preload + 12 warm-up + rows
	const int xo = qx0 * 2 + col;         // this thread's output column
	// rows this work item may store: its chunk, clipped to the band (uniform)
	const int ylo = max( qy0 * 2, P.srow_lo );
	const int yhi = min( qy1 * 2, P.srow_hi );
	const bool xok = ( xo < P.nw );
	const bool strip_full = ( qx0 * 2 + U2_TW <= P.nw );
	const int dlane_b = ( xo * 4 + hf * 2 ) * 4; // byte offset within a row
	const int drow_b = ( IO != 0 ? P.istride_b :
		(int) P.dst_ss * 4 );                // bytes per destination row
	const int srow_b = (int) P.src_ss * ( SRC != 0 ? 1 : 4 ); // bytes per source row

	// Buffer addressing (uniform 128-bit resource + 32-bit lane offset + scalar
	// row offset): a load/store moves ONE address dword per lane instead of a
	// 64-bit flat address -- store issue cost is proportional to the dwords a
	// wave sends to the memory pipeline. Both resources are based at this work
	// item's first row so every offset fits 31 bits for any image size.
	const int ubase = max( u0, P.rmin );
	// (raw sources: a dword-aligned base -- its two low bits go into the lanes'
	// offsets -- and the range the image's bytes end in, rounded up to a dword:
	// a pixel's second dword beyond it reads 0 without touching memory)
	// (the image may end 2 GiB or more above this work item's base: the range
	// is computed in long and stops at the largest one -- the rows this item
	// reads, at most U2_RB * UP2_KMAX of a pitch below 1 << 22, end below it)
	const char* const sbase = (const char*) P.src + (long) ubase * srow_b;
	const int rsh = ( SRC != 0 ? (int) ( (unsigned long long) sbase & 3 ) : 0 );
	const long rend = ( rsh + (long) ( P.rmax - ubase ) * srow_b +
		(long) P.sw * PXB + 3 ) & ~3L;
	const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
		(void*) ( sbase - rsh ), 0, ( SRC != 0 ?
		(int) ( rend < 0x7ffffffcL ? rend : 0x7ffffffcL ) : 0x7fffffff ),
		0x00020000 );
	const __amdgpu_buffer_rsrc_t rdst = __builtin_amdgcn_make_buffer_rsrc(
		(void*) ( P.dst + (long) ( qy0 * 2 - P.dst_row0 ) * P.dst_ss ), 0,
		0x7fffffff, 0x00020000 );

	constexpr bool GSRC = ( SRC / 100 == 3 ); // raw uint8 elements, linearised
	constexpr bool GOUT = up2_gamma_out< IO >; // a de-linearised uint8 result
	static_assert( !GSRC || ( SESZ == 1 && GOUT ),
		"a linearised source is uint8, its result de-linearised" );

	f2 tw[ 8 ];  // ring of the last T values of this column   (slot u & 7)
	f2 cw[ VT ? 1 : 16 ]; // ring of the last C2 values of this column (slot u & 15)
	f2 ea[ VT ? 12 : 1 ]; // VT: running sums of the even output rows (slot q % 12)
	f2 oa[ VT ? 12 : 1 ]; // VT: running sums of the odd output rows  (slot q % 12)

#pragma unroll
	for( int i = 0; i < 8; i++ ) tw[ i ] = (f2) 0.0f;
#pragma unroll
	for( int i = 0; i < ( VT ? 1 : 16 ); i++ ) cw[ i ] = (f2) 0.0f;
#pragma unroll
	for( int i = 0; i < ( VT ? 12 : 1 ); i++ ) ea[ i ] = oa[ i ] = (f2) 0.0f;

	// ---- VT: per-lane addresses, computed ONCE per work item and carried
	// through all phases in 6 registers (LDS byte addresses packed two to a
	// register, unpacked by one volatile instruction where a phase needs one:
	// opaque to the compiler, which would otherwise keep every derived address
	// alive next to the 64 registers of vertical state -- or, as before this
	// change, had to rebuild them from the lane id in every phase: 13 % of the
	// vector instructions of a marching step).
	constexpr int RPI0 = U2_NT / U2_SW;
	constexpr int CN0 = U2_RB * U2_CW;
	unsigned pkA = 0; // lo: H2 stream start in sC; hi: this half pixel in sT
	unsigned pkB = 0; // H1 iterations 0 / 1: first source pixel in sS
	unsigned pkC = 0; // H1 iteration 2: source in sS / destination in sC
	unsigned pkD = 0; // lo: H1 iteration 0's destination in sC; hi: H2's first sum in sT
	int pvoff = -1;   // source byte offset of this lane's DMA pixel (< 0: none)
	int dlv = 0;      // destination byte offset within a row
	int dlv2 = 0;     // IO != 0: ... of the lane's second channel

	if constexpr( VT )
	{
		typedef __attribute__(( address_space( 3 ))) void* lp;
		auto la = []( const void* q ) -> unsigned
			{ return( (unsigned) (unsigned long long) (lp) q ); };

		{
			const int r = tid / U2_SW;
			const int sx = clampi( qx0 - 9 + ( tid - r * U2_SW ), P.sw - 1 );
			pvoff = ( tid < RPI0 * U2_SW ? r * srow_b + sx * PXB + rsh : -1 );
		}

		if constexpr( IO != 0 )
		{
			dlv = ( xo < P.nw && hf * 2 < P.ich ?
				( xo * P.ich + hf * 2 ) * ESZ : (int) 0x80000000u );
			dlv2 = ( xo < P.nw && hf * 2 + 1 < P.ich ?
				( xo * P.ich + hf * 2 + 1 ) * ESZ : (int) 0x80000000u );
		}
		else
		{
			dlv = ( xo < P.nw ? ( xo * 4 + hf * 2 ) * 4 : (int) 0x80000000u );
		}

		// H2's lanes: half pixel, first pixel within its group, row (low two
		// bits), group of 4 * U2_HS pixels; a wave takes four rows. With
		// U2_HS == 4 a 32-lane half of ds_read_b64 is one group x four rows
		// (pitch 704 B: 0, 192, 128, 64 mod 256 B) of 64-byte runs: no bank
		// conflict. (U2_HS == 2: 32-byte runs, 2-way in every lane order.)
		{
			constexpr int LS = ( U2_HS == 4 ? 2 : 1 );
			const int hr = ( tid >> 6 ) * 4 + (( tid >> ( 1 + LS )) & 3 );
			const int hq = (( tid >> ( 3 + LS )) & ( 8 / U2_HS - 1 )) * 4 * U2_HS +
				(( tid >> 1 ) & ( U2_HS - 1 ));

			pkA = la( (const f2*) &sC[ hr * U2_CW + hq ] + hf ) |
				( la( (const f2*) sT + ((( col & 1 ) * U2_TPL + ( col >> 1 )) * 2 +
				hf )) << 16 );
			pkD = la( &sC[ tid ]) |
				( la( (const f2*) &sT[ hr * ( U2_TW / 2 ) + hq ] + hf ) << 16 );
		}

		unsigned ha[ 3 ], hd = 0;
#pragma unroll
		for( int k = 0; k < 3; k++ )
		{
			const int i = min( tid + k * U2_NT, CN0 - 1 );
			const int r = (int) ((unsigned) i / U2_CW );
			ha[ k ] = la( &sS[ i + r * ( U2_SW - U2_CW )]);
			hd = la( &sC[ i ]);
		}

		pkB = ha[ 0 ] | ( ha[ 1 ] << 16 );
		pkC = ha[ 2 ] | ( hd << 16 );
		asm volatile( "" : "+v"( pkA ), "+v"( pkB ), "+v"( pkC ), "+v"( pkD ),
			"+v"( pvoff ), "+v"( dlv ));

		if constexpr( IO != 0 && IO != 6 && IO != 7 )
		{
			asm volatile( "" : "+v"( dlv2 ));
		}
	}

	typedef const __attribute__(( address_space( 3 ))) f4* lds_cf4;
	typedef __attribute__(( address_space( 3 ))) f4* lds_f4;
	typedef const __attribute__(( address_space( 3 ))) f2* lds_cf2;
	typedef __attribute__(( address_space( 3 ))) f2* lds_f2;
	auto lo16 = []( const unsigned v ) -> unsigned
	{
		unsigned r;
		asm volatile( "v_and_b32 %0, 0xffff, %1" : "=v"( r ) : "v"( v ));
		return( r );
	};
	auto hi16 = []( const unsigned v ) -> unsigned
	{
		unsigned r;
		asm volatile( "v_lshrrev_b32 %0, 16, %1" : "=v"( r ) : "v"( v ));
		return( r );
	};

	// ---- source tiles: LDS-DMA (buffer_load_dwordx4 ... lds), HBM -> LDS
	// without passing through registers. One instruction moves whole pixels
	// of U2_RPI consecutive tile rows: lane f takes pixel f % U2_SW of row
	// f / U2_SW, and the hardware writes lane l of a wave to M0 + l * 16, i.e.
	// exactly the flat (row, px) order of sS. The per-lane source offset is
	// loop-invariant; the row group is selected by the scalar offset.
	constexpr int RPI = U2_NT / U2_SW;   // tile rows per DMA instruction
	constexpr int NDMA = U2_RB / RPI;
	static_assert( RPI >= 1 && U2_RB % RPI == 0, "S tile / DMA geometry" );

	typedef __attribute__(( address_space( 3 ))) void* ldsptr;
	const int wave = __builtin_amdgcn_readfirstlane( tid >> 6 );
	const int wave_b = wave * 1024;

	// raw sources: the byte offset (from rsrc's base) of this lane's pixel of
	// DMA instruction k of the tile that starts at row ub; < 0: the lane has none
	auto raw_off = [&]( const int k, const int ub ) -> int
	{
		if( ub >= P.rmin && ub + U2_RB <= P.rmax + 1 )
		{
			return( pvoff >= 0 ? pvoff + ( ub - ubase + k * RPI ) * srow_b : -1 );
		}

		// image top / bottom: rows clamp individually (rare path)
		const int tid = fresh_tid( wave );
		const int pr_r = tid / U2_SW;
		const int pr_sx = clampi( qx0 - 9 + ( tid - pr_r * U2_SW ), P.sw - 1 );
		const int sy = min( max( ub + k * RPI + pr_r, P.rmin ), P.rmax );

		return( tid < RPI * U2_SW ? ( sy - ubase ) * srow_b + pr_sx * PXB + rsh :
			-1 );
	};

	// raw sources: the tile's pixels, DMAed as pairs of dwords, become floats
	// (called by every thread after vmcnt( 0 ), before the closing barrier)
	auto land_raw = [&]( const int ub )
	{
		typedef const __attribute__(( address_space( 3 ))) unsigned* lds_cu;
		unsigned d0[ NDMA ], d1[ NDMA ];
		int off[ NDMA ];
		const int lw = ( threadIdx.x & 63 ) * 4;
#pragma unroll
		for( int k = 0; k < NDMA; k++ )
		{
			off[ k ] = raw_off( k, ub );
			const char* const st = (const char*) sS + k * RPI * U2_SW * 16 +
				wave_b + lw;
			d0[ k ] = *(lds_cu) (const void*) st;
			d1[ k ] = *(lds_cu) (const void*) ( st + 256 );
		}

		// (every read above before any write below: the float pixels go where
		// the wave's own dwords lay)
		asm volatile( "s_waitcnt lgkmcnt(0)" ::: "memory" );
#pragma unroll
		for( int k = 0; k < NDMA; k++ )
		{
			if( off[ k ] >= 0 )
			{
				const unsigned sh = (unsigned) off[ k ] & 3u;
				const unsigned lo = __builtin_amdgcn_alignbyte( d1[ k ], d0[ k ], sh );
				f4 px;

				if( SBF16 )
				{
					// (exact for every bit pattern: the element is the float's
					// upper half)
					const unsigned hi = d1[ k ] >> ( sh * 8 );
					px.x = __uint_as_float( lo << 16 );
					px.y = __uint_as_float( lo & 0xffff0000u );
					px.z = __uint_as_float( hi << 16 );
					px.w = ( SCH == 4 ? __uint_as_float( hi & 0xffff0000u ) : 0.0f );
				}
				else
				if( SHALF )
				{
					const unsigned hi = d1[ k ] >> ( sh * 8 );
					px.x = (float) __builtin_bit_cast( _Float16,
						(unsigned short) ( lo & 0xffffu ));
					px.y = (float) __builtin_bit_cast( _Float16,
						(unsigned short) ( lo >> 16 ));
					px.z = (float) __builtin_bit_cast( _Float16,
						(unsigned short) ( hi & 0xffffu ));
					px.w = ( SCH == 4 ? (float) __builtin_bit_cast( _Float16,
						(unsigned short) ( hi >> 16 )) : 0.0f );
				}
				else
				if constexpr( GSRC )
				{
					// (k_pack_gamma_px< uint8_t, SCH >'s expressions)
					const float* const tbl = ds_table< 256 >();
					const unsigned b0 = lo & 0xffu, b3 = lo >> 24;
					px.x = tbl[ b0 ];
					px.y = tbl[ ( lo >> 8 ) & 0xffu ];
					px.z = tbl[ ( lo >> 16 ) & 0xffu ];
					px.w = 0.0f;

					if constexpr( SCH == 4 )
					{
						px.w = tbl[ b3 ];
						px.x = ( P.G.alpha_index == 0 ? (float) b0 * P.G.gm : px.x );
						px.w = ( P.G.alpha_index == 3 ? (float) b3 * P.G.gm : px.w );
					}
				}
				else
				if( SESZ == 1 )
				{
					px.x = (float) ( lo & 0xffu );
					px.y = (float) (( lo >> 8 ) & 0xffu );
					px.z = (float) (( lo >> 16 ) & 0xffu );
					px.w = ( SCH == 4 ? (float) ( lo >> 24 ) : 0.0f );
				}
				else
				{
					const unsigned hi = d1[ k ] >> ( sh * 8 );
					px.x = (float) ( lo & 0xffffu );
					px.y = (float) ( lo >> 16 );
					px.z = (float) ( hi & 0xffffu );
					px.w = ( SCH == 4 ? (float) ( hi >> 16 ) : 0.0f );
				}

				*(f4*) ((char*) sS + k * RPI * U2_SW * 16 + wave_b + lw * 4 ) = px;
			}
		}
	};

	auto prefetch = [&]( const int ub )
	{
		if constexpr( SRC != 0 )
		{
#pragma unroll
			for( int k = 0; k < NDMA; k++ )
			{
				const int o = raw_off( k, ub );

				if( o >= 0 )
				{
					const ldsptr q = (ldsptr) ((char*) sS + k * RPI * U2_SW * 16 +
						wave_b );
					__builtin_amdgcn_raw_ptr_buffer_load_lds( rsrc, q, 4, o & ~3,
						0, 0, U2_LDAUX );
					__builtin_amdgcn_raw_ptr_buffer_load_lds( rsrc,
						(ldsptr) ((char*) q + 256 ), 4, ( o & ~3 ) + 4, 0, 0,
						U2_LDAUX );
				}
			}

			return;
		}

		if( VT && ub >= P.rmin && ub + U2_RB <= P.rmax + 1 )
		{
			// (interior rows: the lane offset is the persistent one)
			if( pvoff >= 0 )
			{
#pragma unroll
				for( int k = 0; k < NDMA; k++ )
				{
					__builtin_amdgcn_raw_ptr_buffer_load_lds( rsrc,
						(ldsptr) ((char*) sS + k * RPI * U2_SW * 16 + wave_b ),
						16, pvoff, ( ub - ubase + k * RPI ) * srow_b, 0,
						U2_LDAUX );
				}
			}

			return;
		}

		const int tid = ( VT ? fresh_tid( wave ) : (int) threadIdx.x );
		const int pr_r = tid / U2_SW;
		const int pr_sx = clampi( qx0 - 9 + ( tid - pr_r * U2_SW ), P.sw - 1 );
		const bool pr_on = ( tid < RPI * U2_SW );
		const int pr_voff = pr_r * srow_b + pr_sx * 16;

		if( !pr_on )
		{
			return;
		}

		if( ub >= P.rmin && ub + U2_RB <= P.rmax + 1 )
		{
#pragma unroll
			for( int k = 0; k < NDMA; k++ )
			{
				__builtin_amdgcn_raw_ptr_buffer_load_lds( rsrc,
					(ldsptr) ((char*) sS + k * RPI * U2_SW * 16 + wave_b ), 16,
					pr_voff, ( ub - ubase + k * RPI ) * srow_b, 0, U2_LDAUX );
			}
		}
		else
		{
#pragma unroll
			for( int k = 0; k < NDMA; k++ )
			{
				// image top / bottom: rows clamp individually (rare path)
				// (the frame's first / last row -- or a window's: rows outside it
				// only feed results nobody stores, avirhip_band_source_rows)
				const int sy = min( max( ub + k * RPI + pr_r, P.rmin ), P.rmax );
				__builtin_amdgcn_raw_ptr_buffer_load_lds( rsrc,
					(ldsptr) ((char*) sS + k * RPI * U2_SW * 16 + wave_b ), 16,
					( sy - ubase ) * srow_b + pr_sx * 16, 0, 0, U2_LDAUX );
			}
		}
	};

	// ---- H1: C = FIR7 along x, one whole pixel per thread and iteration,
	// flat over the C tile (7 ds_read_b128 + 1 ds_write_b128 per pixel)
	constexpr int CN = U2_RB * U2_CW;
	constexpr int NH1 = ( CN + U2_NT - 1 ) / U2_NT;
	constexpr int H1EVERY = U2_RB / NH1; // woven into every H1EVERY-th V step
	static_assert( NH1 <= U2_RB, "H1 iterations must fit into the marching steps" );
	static_assert( !VT || ( NH1 == 3 && CN == CN0 && RPI == RPI0 ), "VT: packed H1 addresses" );

	auto h1_iter = [&]( const int k, const f2 ( &h )[ 4 ])
	{
		const int i = tid + k * U2_NT;

		if(( k + 1 ) * U2_NT <= CN || i < CN )
		{
			const int r = (int) ((unsigned) i / U2_CW );
			const f4* s = &sS[ i + r * ( U2_SW - U2_CW )];
			const f4 s0 = s[ 0 ], s1 = s[ 1 ], s2 = s[ 2 ], s3 = s[ 3 ];
			const f4 s4 = s[ 4 ], s5 = s[ 5 ], s6 = s[ 6 ];
			f4 a = tmul( h[ 0 ], s3 );
			a = a + tmul( h[ 1 ], s4 + s2 );
			a = a + tmul( h[ 2 ], s5 + s1 );
			a = a + tmul( h[ 3 ], s6 + s0 );
			sC[ i ] = a;
		}
	};

	// the VT form, without a lane condition (no control flow inside a vertical
	// step: basic-block boundaries let the compiler sink accumulation chains
	// across them; lanes past the tile's end redo its last pixel), addresses
	// from the persistent packed registers
	auto h1_iter_p = [&]( const int k, const f2 ( &h )[ 4 ])
	{
		const unsigned sa = ( k == 0 ? lo16( pkB ) : k == 1 ? hi16( pkB ) :
			lo16( pkC ));
		const unsigned da = ( k == 2 ? hi16( pkC ) :
			lo16( pkD ) + k * U2_NT * 16 );
		const lds_cf4 s = (lds_cf4) (unsigned long long) sa;
		const f4 s0 = s[ 0 ], s1 = s[ 1 ], s2 = s[ 2 ], s3 = s[ 3 ];
		const f4 s4 = s[ 4 ], s5 = s[ 5 ], s6 = s[ 6 ];
		f4 a = tmul( h[ 0 ], s3 );
		a = a + tmul( h[ 1 ], s4 + s2 );
		a = a + tmul( h[ 2 ], s5 + s1 );
		a = a + tmul( h[ 3 ], s6 + s0 );
		*(lds_f4) (unsigned long long) da = a;
	};

	// ---- H2: T[2q], T[2q+1] = 12-tap even / odd interpolation of C along x.
	// Transposed form: the bank phase is bit-symmetric, so the product
	// fe[t]*C[m] belongs to even( m+3-t ) and to odd( m-9+t ), outputs of two
	// source pixels 12 - 2t apart. A thread owns one half pixel of the four
	// source pixels q0 + i * U2_HS of one row -- 8 running sums -- and streams
	// once, in ascending order, over the 3 * U2_HS + 13 half pixels
	// C[q0-3 .. q0+3*U2_HS+9]: at stream position k the even sum i takes tap
	// k - i*U2_HS and the odd sum j takes fe[12 - k + j*U2_HS] (its own tap
	// k - j*U2_HS - 1); a tap index wanted by an even and an odd sum at the
	// same position is multiplied once: 81 (U2_HS 4) or 80 (U2_HS 2) packed
	// multiplies for the 96 products. Every sum starts from +0 and receives
	// the same products in the same (ascending tap) order as a sum of its own
	// => same bits. Plain form: one source pixel (two whole output pixels) per
	// thread and iteration from a 13-px window.
	auto h2_phase = [&]()
	{
		if( VT && U2_ON( 2 ))
		{
			const TapsI H = load_taps_i( P.coef );
			const lds_cf2 c = (lds_cf2) (unsigned long long) lo16( pkA );
			const lds_f2 t0 = (lds_f2) (unsigned long long) hi16( pkD );
			constexpr int NP = 3 * U2_HS + 13; // stream positions
			constexpr int PB = U2_H2PB;        // ... per block of LDS reads
			constexpr int NB = ( NP + PB - 1 ) / PB;
			f2 e[ 4 ], o[ 4 ];
			f2 w[ 2 ][ PB ];

#pragma unroll
			for( int i = 0; i < 4; i++ ) e[ i ] = o[ i ] = (f2) 0.0f;
#pragma unroll
			for( int k = 0; k < PB; k++ ) w[ 0 ][ k ] = c[ k * 2 ];

			// the stream in blocks: the next block's reads are in flight
			// while this one is consumed (the transposed vertical phase keeps
			// 64 registers live across this phase)
#pragma unroll
			for( int b = 0; b < NB; b++ )
			{
#pragma unroll
				for( int k = 0; k < PB; k++ )
				{
					if(( b + 1 ) * PB + k < NP )
					{
						w[ ( b + 1 ) & 1 ][ k ] = c[ (( b + 1 ) * PB + k ) * 2 ];
					}
				}

#pragma unroll
				for( int kk = 0; kk < PB; kk++ )
				{
					const int k = b * PB + kk;
#pragma unroll
					for( int t = 0; t < 12; t++ )
					{
						bool any = false;
#pragma unroll
						for( int i = 0; i < 4; i++ )
						{
							any |= ( k < NP && ( k - i * U2_HS == t ||
								12 - k + i * U2_HS == t ));
						}

						if( any )
						{
							const f2 pr = H.fe( t ) * w[ b & 1 ][ kk ];
#pragma unroll
							for( int i = 0; i < 4; i++ )
							{
								if( k - i * U2_HS == t ) e[ i ] = e[ i ] + pr;
								if( 12 - k + i * U2_HS == t ) o[ i ] = o[ i ] + pr;
							}
						}
					}
				}

				// pin the sums that have begun, and the order of the reads,
				// here: the sums are eight independent chains, and nothing
				// else keeps the compiler from issuing the whole stream's
				// reads first (50 registers)
				asm volatile( "" ::: "memory" );
#pragma unroll
				for( int i = 0; i < 4; i++ )
				{
					if( i * U2_HS < ( b + 1 ) * PB ) asm volatile( "" : "+v"( e[ i ]));
					if( i * U2_HS + 1 < ( b + 1 ) * PB ) asm volatile( "" : "+v"( o[ i ]));
				}

				__builtin_amdgcn_sched_barrier( 0 );
			}

#pragma unroll
			for( int i = 0; i < 4; i++ )
			{
				t0[ i * U2_HS * 2 ] = e[ i ];
				t0[ ( U2_TPL + i * U2_HS ) * 2 ] = o[ i ];
			}
		}
		else
		if( U2_ON( 2 ))
		{
			const Taps H = load_taps( P.coef + U2_PAIRED );
			const int tid = ( VT ? fresh_tid( wave ) : (int) threadIdx.x );
			const int qq = tid & ( U2_TW / 2 - 1 );

			for( int r = tid / ( U2_TW / 2 ); r < U2_RB;
				r += U2_NT / ( U2_TW / 2 ))
			{
				const f4* c = &sC[ r * U2_CW + qq ];
				f4 e = (f4) 0.0f;
				f4 o = (f4) 0.0f;
				f4 w[ 13 ];

				if( VT )
				{
					// the window in three parts of 5 + 4 + 4 pixels: the
					// transposed vertical phase keeps 64 registers live
					// across this phase
#pragma unroll
					for( int t = 0; t < 5; t++ ) w[ t ] = c[ t ];
#pragma unroll
					for( int t = 0; t < 4; t++ )
					{
						e = e + tmul( H.fe( t ), w[ t ]);
						o = o + tmul( H.fo( t ), w[ t + 1 ]);
					}

					__builtin_amdgcn_sched_barrier( 0 );
#pragma unroll
					for( int t = 5; t < 9; t++ ) w[ t ] = c[ t ];
#pragma unroll
					for( int t = 4; t < 8; t++ )
					{
						e = e + tmul( H.fe( t ), w[ t ]);
						o = o + tmul( H.fo( t ), w[ t + 1 ]);
					}

					__builtin_amdgcn_sched_barrier( 0 );
#pragma unroll
					for( int t = 9; t < 13; t++ ) w[ t ] = c[ t ];
#pragma unroll
					for( int t = 8; t < 12; t++ )
					{
						e = e + tmul( H.fe( t ), w[ t ]);
						o = o + tmul( H.fo( t ), w[ t + 1 ]);
					}
				}
				else
				{
#pragma unroll
				for( int t = 0; t < 7; t++ ) w[ t ] = c[ t ];
#pragma unroll
				for( int t = 0; t < 6; t++ )
				{
					e = e + tmul( H.fe( t ), w[ t ]);
					o = o + tmul( H.fo( t ), w[ t + 1 ]);
				}

				// second half of the window only now: 13 pixels at once
				// would cost 52 VGPRs
				__builtin_amdgcn_sched_barrier( 0 );
#pragma unroll
				for( int t = 7; t < 13; t++ ) w[ t ] = c[ t ];
#pragma unroll
				for( int t = 6; t < 12; t++ )
				{
					e = e + tmul( H.fe( t ), w[ t ]);
					o = o + tmul( H.fo( t ), w[ t + 1 ]);
				}
				}

				sT[ r * ( U2_TW / 2 ) + qq ] = e;
				sT[ U2_TPL + r * ( U2_TW / 2 ) + qq ] = o;
			}
		}

	};

	// One marching step of U2_RB source rows. R0 = ring phase of its first
	// row (compile-time), so every ring access below is a fixed register.
	auto march = [&]( auto R0C, const int ub, const bool more,
		const bool more2 )
	{
		constexpr int R0 = decltype( R0C )::value;

		// ======== interval B: H2 of this step, while the S tile of the next
		// step lands in sS (nobody reads sS in this interval: H1 of this step
		// ran inside the previous vertical phase). The DMA is complete
		// (vmcnt) before the closing barrier.
		if( more && U2_ON( 8 ))
		{
			prefetch( ub + U2_RB );
		}

		u2_setprio( U2_PRIO_H );
		h2_phase();

		U2_SYNC();
		u2_setprio( U2_PRIO_V );

		// ======== interval A: V of this step, with H1 of the NEXT step woven
		// into it (its LDS latency hides behind the vertical VALU work)
		// ---- V: one half-column per thread, statically unrolled marching.
		// FAST: every row of this step is stored by every lane (interior of
		// the chunk, full strip): no per-row conditions at all.
		const Taps V = load_taps( P.coef + U2_PAIRED + 64 );
		// horizontal FIR taps (4 pairs), parked in VGPRs: the vertical taps
		// already fill the SGPR file
		f2 hv[ 4 ];
		{
			const f8 HF = load_f8( P.coef + U2_PAIRED );
#pragma unroll
			for( int t = 0; t < 4; t++ )
			{
				asm volatile( "v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3"
					: "=&v"( hv[ t ].x ), "=&v"( hv[ t ].y )
					: "s"( HF[ t * 2 ]), "s"( HF[ t * 2 + 1 ]));
			}
		}
		const int yb = ( ub - 9 ) * 2; // output row pair of the step's first row
		int so = ( yb - qy0 * 2 ) * drow_b; // scalar byte offset of row yb

		// this thread's half pixel of T: plane = column parity
		const f2* sT2 = (const f2*) sT +
			((( col & 1 ) * U2_TPL + ( col >> 1 )) * 2 + hf );

		auto vsteps = [&]( auto FASTC )
		{
			constexpr bool FAST = decltype( FASTC )::value;
			tw[ R0 & 7 ] = sT2[ 0 ];
#pragma unroll
			for( int rr = 0; rr < U2_RB; rr++ )
			{
				const int g = R0 + rr; // ring phase of this row

				if( rr + 1 < U2_RB )
				{
					// ring slot (g+1)&7 holds T[u-7], outside the window
					tw[ ( g + 1 ) & 7 ] = sT2[ ( rr + 1 ) * U2_TW ];
				}

				f2 c2 = V.f( 0 ) * tw[ ( g - 3 ) & 7 ];
				c2 = c2 + V.f( 1 ) * ( tw[ ( g - 2 ) & 7 ] +
					tw[ ( g - 4 ) & 7 ]);
				c2 = c2 + V.f( 2 ) * ( tw[ ( g - 1 ) & 7 ] +
					tw[ ( g - 5 ) & 7 ]);
				c2 = c2 + V.f( 3 ) * ( tw[ g & 7 ] + tw[ ( g - 6 ) & 7 ]);
				cw[ g & 15 ] = c2;

				const int y0 = yb + rr * 2;

				if(( FAST || ( y0 + 1 >= ylo && y0 < yhi )) && U2_ON( 4 ))
				{
					f2 e = (f2) 0.0f;
					f2 o = (f2) 0.0f;
#pragma unroll
					for( int t = 0; t < 12; t++ )
					{
						// mul, mul, add, add: a dependent v_pk op needs one
						// issue slot of distance; pin the order so that slot
						// is the other accumulator's op and not an s_nop
						const f2 pe = V.fe( t ) * cw[ ( g - 12 + t ) & 15 ];
						const f2 po = V.fo( t ) * cw[ ( g - 11 + t ) & 15 ];
						__builtin_amdgcn_sched_barrier( 0 );
						e = e + pe;
						o = o + po;
						__builtin_amdgcn_sched_barrier( 0 );
					}

					// uniform row pointer + 32-bit lane byte offset
					if(( FAST || ( xok && y0 >= ylo )) &&
						( U2_ON( 1 ) || e.x == 1234.5f ))
					{
						__builtin_amdgcn_raw_buffer_store_b64(
							__builtin_bit_cast( u2, e ), rdst, dlane_b, so, U2_STAUX );
					}

					if(( FAST || ( xok && y0 + 1 < yhi )) &&
						( U2_ON( 1 ) || o.y == 1234.5f ))
					{
						__builtin_amdgcn_raw_buffer_store_b64(
							__builtin_bit_cast( u2, o ), rdst, dlane_b,
							so + drow_b, U2_STAUX );
					}
				}

				so += 2 * drow_b;

				// ---- H1 of the next step, one iteration
				if( rr % H1EVERY == 0 && rr / H1EVERY < NH1 && more &&
					U2_ON( 2 ))
				{
					h1_iter( rr / H1EVERY, hv );
				}
			}
		};

		if( strip_full && yb >= ylo && yb + 2 * U2_RB <= yhi )
		{
			vsteps( std::true_type() );
		}
		else
		{
			vsteps( std::false_type() );
		}

		U2_SYNC();
	};

	prefetch( u0 );

	// the gamma kinds' tables: the plan's, copied by the workgroup's threads
	if constexpr( GSRC )
	{
		for( int i = tid; i < 256; i += U2_NT )
		{
			ds_table< 256 >()[ i ] = P.G.tbl[ i ];
		}
	}

	if constexpr( GOUT )
	{
		for( int i = tid; i < U2_GTHR; i += U2_NT )
		{
			ds_table< U2_GTHR >()[ i ] = P.G.thr[ i ];
		}
	}

	if constexpr( SRC != 0 )
	{
		if constexpr( GSRC )
		{
			U2_SYNC(); // (the first tile's conversion reads the whole table)
		}

		AVIRHIP_WAIT_VM( 0 );
		land_raw( u0 );
	}

	U2_SYNC();

	{
		// H1 of the first tile (later tiles: woven into the vertical phase)
		const f4 HF = load_f4( P.coef );
		f2 hp[ 4 ];
#pragma unroll
		for( int t = 0; t < 4; t++ )
		{
			hp[ t ] = splat( HF[ t ]);
		}

#pragma unroll
		for( int k = 0; k < NH1; k++ )
		{
			h1_iter( k, hp );
		}
	}

	U2_SYNC();

	if constexpr( VT )
	{
		// ---- transposed vertical phase. Ring phase g of a row: tw slot g & 7,
		// running sums even( q ) / odd( q ) in slot q % 12 with q counted so that
		// the row of phase g carries C2 index m = g (mod 12): the product
		// fe[t]*C2[m] goes to even( m+3-t ) and odd( m-9+t ); even( m+3 ) and
		// odd( m+2 ) start on this row (0 + product), even( m-8 ) and
		// odd( m-9 ) are complete after it: output rows y0 + 2 and y0 + 1.
		// MODE 2: first 24 rows of the chunk (row j = g of the chunk: sums of
		// rows before the chunk are neither updated nor stored).
		// MODE 3 (U2_TAIL, up2_chunks.h): the chunk's last step, from the
		// fourth step on. The step's last row carries m = qe + 8, where
		// 2 * qe = yb + 16 is the first output row after the step, so row rr
		// carries m = qe + 1 + rr, and even( m+3-t ) / odd( m-9+t ) are output
		// rows below 2 * qe only for t >= rr + 5 / t <= 7 - rr. The other sums
		// are rows of the chunk above: neither updated nor started (68 + 60
		// adds, 36 multiplies whose two sums are both unwanted: 124 packed
		// instructions of the steady 288 remain), row yb + 16 has no store,
		// and no H1 is woven in: there is no next step to read it. A chunk
		// that the frame's end clips (by fewer than 8 row pairs) needs no case
		// of its own: its end lies before 2 * qe, so the rule only keeps more
		// than needed. So with bands and windows: ylo / yhi clip the stores,
		// not the march. One code
		// variant per ring phase: whether a row is stored is one scalar bit
		// test, and lanes right of the image carry an out-of-range buffer
		// offset (the hardware drops their stores).
		static_assert( !VT || U2_RB == 8, "VT marching period is 3 x 8 rows" );
#ifdef U2_DBG
		int abl_tail = 0; // (ablation bit 32: this step's woven H1 feeds a skipped H2)
#endif
		void* const dbase = ( IO != 0 ? (void*) ( (char*) P.ibase +
			(long) ( qy0 * 2 - P.dst_row0 ) * P.istride_b ) :
			(void*) ( P.dst + (long) ( qy0 * 2 - P.dst_row0 ) * P.dst_ss ));

		// (the caller's pixels, IO != 0: `store_io`, `store_g`)
#include "up2_store.inl"

		// (a row's products and the sums they go to, by MODE: `vinterp`)
#include "up2_vt.inl"

		auto vstep_t = [&]( auto R0C, auto MODEC, const int ub,
			const bool more )
		{
			constexpr int R0 = decltype( R0C )::value;
			constexpr int MODE = decltype( MODEC )::value;
			const TapsE V = load_taps_e( P.coef + 32 );
			// the horizontal FIR taps stay in SGPRs too (16 + 4 taps in all,
			// 10 pairs)
			f2 hv[ 4 ];
			{
				const f4 HF = load_f4( P.coef );
#pragma unroll
				for( int t = 0; t < 4; t++ )
				{
					hv[ t ] = splat( HF[ t ]);
				}
			}

			const int yb = ( ub - 9 ) * 2;
			int so = ( yb - qy0 * 2 ) * drow_b; // scalar byte offset of row yb
			const int dlane_v = dlv;
			const lds_cf2 sT2 = (lds_cf2) (unsigned long long) hi16( pkA );
			// rows yb + 1 .. yb + 16 that lie in [ylo, yhi)
			const int rlo = min( max( ylo - ( yb + 1 ), 0 ), 2 * U2_RB );
			const int rhi = min( max( yhi - ( yb + 1 ), 0 ), 2 * U2_RB );
			const unsigned rmask = __builtin_amdgcn_readfirstlane(
				(( 1u << rhi ) - 1u ) & ~(( 1u << rlo ) - 1u ));

			tw[ R0 & 7 ] = sT2[ 0 ];
#pragma unroll
			for( int rr = 0; rr < U2_RB; rr++ )
			{
				const int g = R0 + rr; // ring phase of this row (0..23)

				if( rr + 1 < U2_RB )
				{
					tw[ ( g + 1 ) & 7 ] = sT2[ ( rr + 1 ) * U2_TW ];
				}

				f2 c2 = V.f( 0 ) * tw[ ( g - 3 ) & 7 ];
				c2 = c2 + V.f( 1 ) * ( tw[ ( g - 2 ) & 7 ] +
					tw[ ( g - 4 ) & 7 ]);
				c2 = c2 + V.f( 2 ) * ( tw[ ( g - 1 ) & 7 ] +
					tw[ ( g - 5 ) & 7 ]);
				c2 = c2 + V.f( 3 ) * ( tw[ g & 7 ] + tw[ ( g - 6 ) & 7 ]);

				if( U2_ON( 4 ))
				{
					vinterp( MODEC, V, c2, g, rr );
					// pin the 24 sums here: the instruction-selection DAG is
					// free to postpone an add until its sum is next used (a
					// row later), keeping the product alive instead -- that
					// spilled ~300 registers
					// (the pruned tail pins the sums it still wants one by
					// one, in vinterp: pinned together, the unwanted ones keep
					// their registers to the end, and two of the three tail
					// bodies spilled 9 to 13 VGPRs)
					if constexpr( MODE != 3 || U2_TAIL < 2 )
					{
					asm volatile( "" : "+v"( ea[ 0 ]), "+v"( ea[ 1 ]),
						"+v"( ea[ 2 ]), "+v"( ea[ 3 ]), "+v"( ea[ 4 ]),
						"+v"( ea[ 5 ]), "+v"( ea[ 6 ]), "+v"( ea[ 7 ]),
						"+v"( ea[ 8 ]), "+v"( ea[ 9 ]), "+v"( ea[ 10 ]),
						"+v"( ea[ 11 ]));
					asm volatile( "" : "+v"( oa[ 0 ]), "+v"( oa[ 1 ]),
						"+v"( oa[ 2 ]), "+v"( oa[ 3 ]), "+v"( oa[ 4 ]),
						"+v"( oa[ 5 ]), "+v"( oa[ 6 ]), "+v"( oa[ 7 ]),
						"+v"( oa[ 8 ]), "+v"( oa[ 9 ]), "+v"( oa[ 10 ]),
						"+v"( oa[ 11 ]));
					}

					const f2 od = oa[ ( g + 3 ) % 12 ]; // odd( m-9 ): row y0 + 1
					const f2 ed = ea[ ( g + 4 ) % 12 ]; // even( m-8 ): row y0 + 2
					// (the pruned tail's last even row is no row of the chunk)
					const bool est = ( MODE != 3 || U2_TAIL < 2 || rr + 1 < U2_RB );

					if( MODE != 2 || g >= 17 )
					{
						// bit k of rmask: row yb + 1 + k is stored by this item.
						// No branches (they would let the compiler sink whole
						// accumulation chains into them): an unwanted row goes
						// through a zero-length view of the destination, whose
						// range check drops the store.
						if constexpr( GOUT )
						{
							const __amdgpu_buffer_rsrc_t r1 =
								__builtin_amdgcn_make_buffer_rsrc( dbase, 0,
								( rmask & ( 1u << ( 2 * rr )) ? 0x7fffffff : 0 ),
								0x00020000 );
							const __amdgpu_buffer_rsrc_t r2 =
								__builtin_amdgcn_make_buffer_rsrc( dbase, 0,
								( rmask & ( 2u << ( 2 * rr )) ? 0x7fffffff : 0 ),
								0x00020000 );

							store_g( od, ed, est, r1, r2, so );
						}
						else
						if constexpr( IO != 0 )
						{
							store_io( od, __builtin_amdgcn_make_buffer_rsrc(
								dbase, 0, ( rmask & ( 1u << ( 2 * rr )) ?
								0x7fffffff : 0 ), 0x00020000 ), so + drow_b );
							if( est )
							store_io( ed, __builtin_amdgcn_make_buffer_rsrc(
								dbase, 0, ( rmask & ( 2u << ( 2 * rr )) ?
								0x7fffffff : 0 ), 0x00020000 ), so + 2 * drow_b );
						}
						else
						{
						if( U2_ON( 1 ) || od.x == 1234.5f )
						{
							__builtin_amdgcn_raw_buffer_store_b64(
								__builtin_bit_cast( u2, od ),
								__builtin_amdgcn_make_buffer_rsrc( dbase, 0,
								( rmask & ( 1u << ( 2 * rr )) ? 0x7fffffff : 0 ),
								0x00020000 ), dlane_v, so + drow_b, U2_STAUX );
						}

						if( est && ( U2_ON( 1 ) || ed.y == 1234.5f ))
						{
							__builtin_amdgcn_raw_buffer_store_b64(
								__builtin_bit_cast( u2, ed ),
								__builtin_amdgcn_make_buffer_rsrc( dbase, 0,
								( rmask & ( 2u << ( 2 * rr )) ? 0x7fffffff : 0 ),
								0x00020000 ), dlane_v, so + 2 * drow_b, U2_STAUX );
						}
						}
					}
				}

				so += 2 * drow_b;
				// (one running offset in one SGPR: the compiler otherwise keeps
				// so + k * drow_b of every row of the ring period in SGPRs of
				// their own -- 30 of them, spilled into VGPR lanes)
				asm volatile( "" : "+s"( so ));

				// ---- H1 of the next step, one iteration
				// (MODE 3 has no next step; a last step in another mode works
				// on stale tiles and nobody reads its result)
				if( rr % H1EVERY == 0 && rr / H1EVERY < NH1 && U2_ON( 2 ) &&
					U2_ABL_H1( rr / H1EVERY ) && U2_ABL_TAIL() && MODE != 3 )
				{
					h1_iter_p( rr / H1EVERY, hv );
				}
			}
		};

		typedef std::integral_constant< int, 0 > I0;
		typedef std::integral_constant< int, 1 > I1;
		typedef std::integral_constant< int, 2 > I2;
		typedef std::integral_constant< int, 3 > I3;
		typedef std::integral_constant< int, 8 > I8;
		typedef std::integral_constant< int, 16 > I16;

		// one marching step: interval B = {DMA of the next S tile, H2 of this
		// step}, interval A = {V of this step, H1 of the next} (see march).
		// MODE 3 is the chunk's last step by construction: no next tile.
		auto march_t = [&]( auto R0C, auto MODEC, const int sb )
		{
			const int ub = u0 + sb;
			const bool more = ( decltype( MODEC )::value != 3 &&
				sb + U2_RB < nsteps );
#ifdef U2_DBG
			// (bit 32: H2 of the chunk's last two steps and the H1 that feeds
			// them -- woven into the step before -- are skipped)
			const bool tail_h2 = (( P.dbg & 32 ) && sb + 2 * U2_RB >= nsteps &&
				nsteps > 6 * U2_RB );
			abl_tail = (( P.dbg & 32 ) && sb + 3 * U2_RB >= nsteps &&
				sb + U2_RB < nsteps && nsteps > 6 * U2_RB ? 1 : 0 );
#endif

			if( more && U2_ON( 8 ))
			{
				prefetch( ub + U2_RB );
			}

#ifdef U2_DBG
			// (bit 1024: wave priority by interval from the bits -- timing
			// experiments, results unchanged: bits 6-7 the priority of the
			// horizontal interval, bits 8-9 that of the vertical one)
			u2_setprio( P.dbg & 1024 ? ( P.dbg >> 6 ) & 3 : U2_PRIO_H );

			if( !tail_h2 )
#else
			u2_setprio( U2_PRIO_H );
#endif
			h2_phase();

			if constexpr( SRC != 0 )
			{
				if( more )
				{
					AVIRHIP_WAIT_VM( 0 );
					land_raw( ub + U2_RB );
				}
			}

			U2_SYNC();
#ifdef U2_DBG
			u2_setprio( P.dbg & 1024 ? ( P.dbg >> 8 ) & 3 : U2_PRIO_V );
#else
			u2_setprio( U2_PRIO_V );
#endif

			vstep_t( R0C, MODEC, ub, more );
			U2_SYNC();
		};

		// the chunk's first 24 rows (nsteps >= 24: cq >= 6), then the period
		// of 24 rows = 3 steps per trip
		march_t( I0(), I2(), 0 );
		march_t( I8(), I2(), 8 );
		march_t( I16(), I2(), 16 );

		// U2_TAIL: the loop leaves the chunk's last step to the tail bodies
		// behind it, one per ring phase. Inside the loop -- as one arm of a
		// branch after H2, or as a whole step that breaks out -- the tail
		// cost every instance 60 to 177 spilled VGPRs: the loop holds
		// lane-dependent branches, so its control flow is made structured as
		// a whole, the way out becomes a flag, and the sums stay live on a
		// path from the tail back into the loop that is never taken.
		constexpr int LAST = ( U2_TAIL >= 1 ? U2_RB : 0 );

		for( int sb = 24; sb + LAST < nsteps; sb += 24 )
		{
			march_t( I0(), I1(), sb );

			if( sb + 8 + LAST >= nsteps )
			{
				break;
			}

			march_t( I8(), I1(), sb + 8 );

			if( sb + 16 + LAST >= nsteps )
			{
				break;
			}

			march_t( I16(), I1(), sb + 16 );
		}

		if( U2_TAIL >= 1 && nsteps > 24 )
		{
			const int sbl = ( nsteps - 1 ) & ~( U2_RB - 1 ); // the last step

			switch(( sbl >> 3 ) % 3 )
			{
				case 0: march_t( I0(), I3(), sbl ); break;
				case 1: march_t( I8(), I3(), sbl ); break;
				default: march_t( I16(), I3(), sbl );
			}
		}
	}
	else
	{
		// the ring period is 16 rows: 16 / U2_RB marching steps per trip
		for( int sb = 0; sb < nsteps; sb += 16 )
		{
#if U2_RB == 16
			march( std::integral_constant< int, 0 >(), u0 + sb, sb + 16 < nsteps,
				sb + 32 < nsteps );
#else
			march( std::integral_constant< int, 0 >(), u0 + sb, sb + 8 < nsteps,
				sb + 16 < nsteps );

			if( sb + 8 >= nsteps )
			{
				break;
			}

			march( std::integral_constant< int, 8 >(), u0 + sb + 8,
				sb + 16 < nsteps, sb + 24 < nsteps );
#endif
		}
	}

#ifdef U2_DBG
	if( tid == 0 && P.clk != nullptr )
	{
		P.clk[ blockIdx.x * 4 ] = clock64() - dbg_c0;
		P.clk[ blockIdx.x * 4 + 1 ] = dbg_w0;
		P.clk[ blockIdx.x * 4 + 2 ] = wall_clock64();
		P.clk[ blockIdx.x * 4 + 3 ] =
			(unsigned) __builtin_amdgcn_s_getreg(( 31 << 11 ) | 4 ) |
			((unsigned long long) __builtin_amdgcn_s_getreg(( 31 << 11 ) | 20 ) << 32 );
	}
#endif
}

// ---------------------------------------------------------------------
// host side: recognise the plan shape and extract the 28 taps per axis
// ---------------------------------------------------------------------

struct Up2Axis
{
	float f[ 4 ], fe[ 12 ], fo[ 12 ];
};

static bool match_axis( const LAxis& ax, Up2Axis& A )
{
	if( ax.ops.size() != 2 || ax.dst_len != ax.src_len * 2 )
	{
		return( false );
	}

	const LOp& a = ax.ops[ 0 ];
	const LOp& g = ax.ops[ 1 ];

	if( a.type != OP_FIR || a.view != VIEW_CLAMP || a.rf != 1 || a.lat != 3 ||
		a.e != 3 || a.in_len != ax.src_len || a.out_len != ax.src_len + 6 ||
		g.type != OP_GATHER || g.view != VIEW_ZS || g.maxtaps != 12 ||
		g.in_len != a.out_len || g.out_len != ax.dst_len )
	{
		return( false );
	}

	for( int i = 0; i < 4; i++ )
	{
		A.f[ i ] = a.h_flt[ i ];
	}

	for( int t = 0; t < 12; t++ )
	{
		A.fe[ t ] = g.h_coef[ t ];
		A.fo[ t ] = g.h_coef[ 12 + t ];
	}

	for( int j = 0; j < g.out_len; j++ )
	{
		const int q = j >> 1;
		const int st = ( j & 1 ? q - 2 : q - 3 );
		const float* cf = &g.h_coef[ (size_t) j * 12 ];
		const float* rf = ( j & 1 ? A.fo : A.fe );

		if( g.h_start[ j ] != st || g.h_ntaps[ j ] != 12 ||
			st + 11 > g.zs_mmax || memcmp( cf, rf, 12 * sizeof( float )) != 0 )
		{
			return( false );
		}
	}

	return( true );
}

struct Up2Data
{
	Up2Axis h, v;
	float* d_coef;
	bool vsym; // vertical bank phase bit-symmetric: fo[t] == fe[11-t]
	bool hsym; // ... and the horizontal one
	bool gain16; // samples within [-1, 1] give sums within [-16, 16] (IO 9)
};

// Whether the plan runs the transposed form k_up2< true, ... >: both axes'
// tap products are shared between an even and an odd sum there.
static bool up2_vt( const avirhip_plan* p, const Up2Data* D )
{
	static const bool novt = ( getenv( "AVIRHIP_UP2_NOVT" ) != nullptr );

	return( D != nullptr && U2_RB == 8 && D -> vsym && D -> hsym && !novt &&
		!( p -> variant & AVIRHIP_VARIANT_UP2_PLAIN_V ));
}

int up2_prepare( avirhip_plan* p )
{
	p -> up2 = nullptr;

	if( p -> is_lancir || p -> ch != 4 )
	{
		return( AVIRHIP_OK );
	}

	Up2Data* D = new Up2Data();

	if( match_axis( p -> h, D -> h ) && match_axis( p -> v, D -> v ))
	{
		// the kernel's tap blocks, packed and paired (Up2Params::coef, Taps)
		float hc[ U2_PAIRED + 128 ] = { 0 };
		const Up2Axis* ax[ 2 ] = { &D -> h, &D -> v };

		for( int a = 0; a < 2; a++ )
		{
			float* o = hc + a * 32;
			memcpy( o, ax[ a ] -> f, 4 * sizeof( float ));
			memcpy( o + 4, ax[ a ] -> fe, 12 * sizeof( float ));
			memcpy( o + 16, ax[ a ] -> fo, 12 * sizeof( float ));
			o = hc + U2_PAIRED + a * 64;

			for( int i = 0; i < 4; i++ )
			{
				o[ 2 * i ] = o[ 2 * i + 1 ] = ax[ a ] -> f[ i ];
			}

			for( int t = 0; t < 12; t++ )
			{
				o[ 8 + 2 * t ] = o[ 9 + 2 * t ] = ax[ a ] -> fe[ t ];
				o[ 32 + 2 * t ] = o[ 33 + 2 * t ] = ax[ a ] -> fo[ t ];
			}
		}

		void* q = nullptr;
		AVIRHIP_HIPCHECK( hipMalloc( &q, sizeof( hc )));
		p -> allocs.push_back( q );
		AVIRHIP_HIPCHECK( hipMemcpy( q, hc, sizeof( hc ),
			hipMemcpyHostToDevice ));
		D -> d_coef = (float*) q;
		D -> vsym = true;
		D -> hsym = true;

		for( int t = 0; t < 12; t++ )
		{
			D -> vsym &= ( memcmp( &D -> v.fo[ t ], &D -> v.fe[ 11 - t ],
				sizeof( float )) == 0 );
			D -> hsym &= ( memcmp( &D -> h.fo[ t ], &D -> h.fe[ 11 - t ],
				sizeof( float )) == 0 );
		}

		D -> gain16 = ( up2_axis_gain( D -> h.f, D -> h.fe, D -> h.fo ) *
			up2_axis_gain( D -> v.f, D -> v.fe, D -> v.fo ) <= 15.0 );
		p -> up2 = D;
		p -> fused_ok |= 4;
		p -> auto_path = 4;
	}
	else
	{
		delete D;
	}

	return( AVIRHIP_OK );
}

void up2_release( avirhip_plan* p )
{
	delete (Up2Data*) p -> up2;
	p -> up2 = nullptr;
}

// The gamma plan whose uint8 result the kernel de-linearises and stores itself:
// the thresholds of the output stage exist, the float pipeline
static bool up2_gamma_u8( const avirhip_plan* p )
{
	return( p -> gamma && p -> out_type == AVIRHIP_U8 &&
		p -> d_gthr != nullptr && !p -> fp4 && !p -> f64 );
}

// up2_run's `io` of a gamma plan (any other keeps its own): 8, or 9 behind a
// uint8 / uint16 source when `gain16` (up2_params.h); 0: none the kernel stores
static int up2_gamma_io( const avirhip_plan* p, const int io, const bool gain16 )
{
	if( !p -> gamma )
	{
		return( io );
	}

	return( !up2_gamma_u8( p ) ? 0 : ( gain16 && ( p -> in_type == AVIRHIP_U8 ||
		p -> in_type == AVIRHIP_U16 ) ? 9 : 8 ));
}

// Whether the plan's marching kernel can store the caller's pixels itself
// (up2_run's `iout`): the transposed vertical phase, default ditherer, and
// without gamma uint8 / uint16 without bit-depth truncation, float pixels of
// 1-3 channels or half / bfloat16 RGBA pixels (such pixels of 1-3 channels
// leave through the output stage); with gamma uint8 pixels (up2_gamma_u8).
bool up2_stores_io( const avirhip_plan* p )
{
	const Up2Data* D = (const Up2Data*) p -> up2;

	if( p -> gamma )
	{
		return( up2_vt( p, D ) && p -> dither == AVIRHIP_DITHER_DEF &&
			up2_gamma_u8( p ));
	}

	return( up2_vt( p, D ) &&
		p -> dither == AVIRHIP_DITHER_DEF &&
		(( p -> out_type == AVIRHIP_U8 && p -> tr_mul == 1.0 &&
		p -> pk_out == 255.0 ) ||
		( p -> out_type == AVIRHIP_U16 && p -> tr_mul == 1.0 &&
		p -> pk_out == 65535.0 ) ||
		( p -> out_type == AVIRHIP_F32 && p -> io_ch < 4 ) ||
		( dtype_is_float16_kind( p -> out_type ) && p -> io_ch == 4 )));
}

// The float RGBA call up2_run cannot refuse (its own checks, io == 0): a source
// window may then be handed over as a virtual frame base.
bool up2_takes_window( const avirhip_plan* p, const void* src, const void* dst )
{
	return( p -> up2 != nullptr && !p -> is_lancir && p -> ch == 4 &&
		p -> io_ch == 4 && p -> in_type == AVIRHIP_F32 &&
		p -> out_type == AVIRHIP_F32 && !p -> gamma &&
		( (uintptr_t) src & 15 ) == 0 && ( (uintptr_t) dst & 7 ) == 0 &&
		( p -> src_stride & 3 ) == 0 &&
		(long) p -> src_stride * 4 < ( 1L << 22 ) &&
		(long) p -> new_w * 16 < ( 1L << 22 ));
}

// `iout` != nullptr: the caller's image (the band's first row) -- uint8 /
// uint16 without bit-depth truncation, or float pixels of 1-3 channels: the
// vertical phase converts and stores there (no float result, no epilogue
// pass); returns 1 if this plan's form of the kernel cannot (the caller then
// runs with a float result).
// `raw` != nullptr (with `iout`): the caller's integer image (uint8 / uint16,
// 3 or 4 channels) instead of `src`; returns 1 if this call cannot take it
// (the caller then packs and calls again).
int up2_run( avirhip_plan* p, const float* src, long src_stride, float* dst,
	int row0, int row1, hipStream_t st, SrcWindow win, const ImageRef* rawimg,
	void* iout )
{
	const void* const raw = ( rawimg != nullptr ? rawimg -> ptr : nullptr );
	const long raw_stride = ( rawimg != nullptr ? rawimg -> stride : 0 );
	const Up2Data* D = (const Up2Data*) p -> up2;
	int io = 0;

	if( iout != nullptr )
	{
		const bool vt = up2_vt( p, D );

		io = ( p -> out_type == AVIRHIP_U8 && p -> tr_mul == 1.0 &&
			p -> pk_out == 255.0 ? 1 :
			( p -> out_type == AVIRHIP_U16 && p -> tr_mul == 1.0 &&
			p -> pk_out == 65535.0 && ( (uintptr_t) iout & 1 ) == 0 ? 2 :
			( p -> out_type == AVIRHIP_F32 && p -> io_ch < 4 &&
			( (uintptr_t) iout & 3 ) == 0 ? 3 :
			( p -> out_type == AVIRHIP_F16 && p -> io_ch == 4 &&
			( (uintptr_t) iout & 3 ) == 0 ? 6 :
			( p -> out_type == AVIRHIP_BF16 && p -> io_ch == 4 &&
			( (uintptr_t) iout & 3 ) == 0 ? 7 : 0 )))));

		// (a gamma plan: 8 / 9, the de-linearised uint8 result, or none)
		if( !vt || ( io = up2_gamma_io( p, io, D -> gain16 )) == 0 ||
			p -> dither != AVIRHIP_DITHER_DEF )
		{
			return( 1 );
		}

		// an integer image in (the pack pass' float copy of it): every sum
		// is finite and small
		if(( io == 1 || io == 2 ) && ( p -> in_type == AVIRHIP_U8 ||
			p -> in_type == AVIRHIP_U16 ))
		{
			io += 3;
		}
	}

	// the integer image as it lies (k_up2< true, IO, SRC >): results of
	// integer sources only (io 4 / 5), whole frames behind the pointer, every
	// pixel inside two aligned dwords (uint16 RGBA: dword-aligned rows)
	// ... or the half / bfloat16 RGBA image, stored as the same type (io 6 /
	// 7), under uint16 RGBA's conditions
	int srck = 0;

	if( raw != nullptr )
	{
		// (1 half, 2 bfloat16: the io code of the same type is 5 + that)
		const int f16kind = ( p -> in_type == AVIRHIP_F16 ? 1 :
			( p -> in_type == AVIRHIP_BF16 ? 2 : 0 ));
		const int esz = ( p -> in_type == AVIRHIP_U8 ? 1 : 2 );
		const long sb = raw_stride * esz;

		if(( f16kind ? io != 5 + f16kind || p -> io_ch != 4 :
			!up2_int_raw_ok( p, io )) || // (io 4 / 5; a gamma plan: 9, uint8)
			( p -> io_ch != 3 && p -> io_ch != 4 ) ||
			win.rows > 0 || ( (uintptr_t) raw & ( esz - 1 )) ||
			( esz == 2 && p -> io_ch == 4 && (( (uintptr_t) raw | sb ) & 3 )) ||
			sb >= ( 1L << 22 ) || getenv( "AVIRHIP_UP2_NO_RAW" ) != nullptr )
		{
			return( 1 );
		}

		srck = ( p -> gamma ? 300 : f16kind * 100 ) + esz * 10 + p -> io_ch;
		src = (const float*) raw;
		src_stride = sb;
	}

	// source pixels travel as 16-byte LDS-DMA pieces, destination half-pixels
	// as 8-byte stores
	if( D == nullptr || ( srck == 0 && (( (uintptr_t) src & 15 ) ||
		( src_stride & 3 ))) || ( io == 0 && ( (uintptr_t) dst & 7 )))
	{
		return( 1 );
	}

	if( row1 <= row0 )
	{
		return( AVIRHIP_OK );
	}

	// the kernel addresses rows with 32-bit float offsets
	if(( srck == 0 && (long) src_stride * 4 >= ( 1L << 22 )) ||
		(long) p -> new_w * 16 >= ( 1L << 22 ))
	{
		return( 1 );
	}

	Up2Params P;
	P.src = src; P.src_ss = src_stride; P.sw = p -> src_w; P.sh = p -> src_h;
	P.rmin = ( win.rows > 0 ? win.first : 0 );
	P.rmax = ( win.rows > 0 ? win.first + win.rows : p -> src_h ) - 1;
	P.dst = dst; P.dst_ss = (long) p -> new_w * 4; P.dst_row0 = row0;
	P.nw = p -> new_w; P.nh = p -> new_h;
	P.srow_lo = row0; P.srow_hi = row1;
	P.nstrips = ( p -> new_w + U2_TW - 1 ) / U2_TW;
	P.ibase = iout; P.ich = p -> io_ch;
	P.istride_b = p -> new_w * p -> io_ch * ( io == 1 || io == 4 || io >= 8 ? 1 :
		( io == 2 || io == 5 || io == 6 || io == 7 ? 2 : 4 ));

	// Chunk heights (up2_chunks.h). A chunk of h source rows costs
	// ( h + 18 ) / U2_RB marching steps (6 rows of preload + 12 of warm-up), so
	// heights U2_RB * k - 18 waste nothing. The band's steps are dealt over n
	// chunks as evenly as they go: the first nlong chunks of a strip are one
	// step taller than the rest, none is left short. n is the count of the
	// least modelled cost: the kernel is VALU-bound and a CU shares its VALUs
	// among its resident workgroups (up to 8), so a launch whose items are all
	// resident at once ends when its most loaded CU does (up2_split_cost; the
	// fit: profiles/up2_chunks/). The split lies on the frame's grid (chunk 0
	// starts at source row 0) whichever band is asked for.
	const int rows = ( row1 - 1 ) / 2 - row0 / 2 + 1; // source rows of the band
	Up2Split sp = up2_split_choose( rows, P.nstrips );

	// sweeps (tools/cq_sweep.sh, tools/up2_chunk_sweep.py): a uniform height,
	// or the balanced split of a given chunk count
	const char* ecq = getenv( "AVIRHIP_UP2_CQ" );
	const char* enc = getenv( "AVIRHIP_UP2_NCHUNKS" );

	if( ecq != nullptr && atoi( ecq ) >= 6 )
	{
		sp.cq = (( atoi( ecq ) + 18 + U2_RB - 1 ) / U2_RB ) * U2_RB - 18;
		sp.nlong = 0;
	}
	else
	if( enc != nullptr && atoi( enc ) >= 1 &&
		up2_split_n( rows, atoi( enc ), 4 ).n != 0 )
	{
		sp = up2_split_n( rows, atoi( enc ), 4 );
	}

	P.cq = sp.cq;
	P.nlong = sp.nlong;
	P.chunk0 = up2_chunk_of( row0 / 2, P.cq, P.nlong );
	const int chunk1 = up2_chunk_of(( row1 - 1 ) / 2, P.cq, P.nlong );

	P.coef = D -> d_coef;
#ifdef U2_DBG
	P.dbg = ( getenv( "AVIRHIP_UP2_DBG" ) != nullptr ?
		atoi( getenv( "AVIRHIP_UP2_DBG" )) : 0 );
	static unsigned long long* dclk = nullptr;
	static int dclk_calls = 0;

	if( dclk == nullptr )
	{
		(void) hipMalloc( &dclk, 8192 * 32 );
	}

	P.clk = dclk;
#endif

	P.nchunks = chunk1 - P.chunk0 + 1;
	const int items = P.nstrips * P.nchunks;

	if( getenv( "AVIRHIP_VERBOSE" ) != nullptr )
	{
		int nb = -1;
		(void) hipOccupancyMaxActiveBlocksPerMultiprocessor( &nb,
			(const void*) k_up2< false, 0 >, U2_NT, 0 );
		fprintf( stderr, "k_up2: %d items (strips %d, cq %d, nlong %d), "
			"occupancy API %d workgroups/CU\n", items, P.nstrips, P.cq,
			P.nlong, nb );
	}

	const char* pad = getenv( "AVIRHIP_UP2_LDSPAD" ); // residency experiments
	const int ldspad = ( pad != nullptr ? atoi( pad ) : 0 );
	if( io >= 8 )
	{
		Up2GParams PG;
		(Up2Params&) PG = P;
		up2_gamma_params( p, PG.G );
#if U2_RB == 8 // (up2_vt: no other build comes here)
#define U2_GAMMA( IOK, SK ) hipLaunchKernelGGL(( k_up2< true, IOK, SK > ), \
	dim3( items ), dim3( U2_NT ), ldspad, st, PG )
		switch( srck )
		{
			case 313: U2_GAMMA( 9, 313 ); break;
			case 314: U2_GAMMA( 9, 314 ); break;
			default:
				if( io == 9 ) U2_GAMMA( 9, 0 );
				else U2_GAMMA( 8, 0 );
		}
#undef U2_GAMMA
#else
		return( 1 );
#endif
	}
	else
	if( srck != 0 )
	{
#define U2_RAW( IOK, SK ) hipLaunchKernelGGL(( k_up2< U2_RB == 8, \
	U2_RB == 8 ? IOK : 0, U2_RB == 8 ? SK : 0 > ), dim3( items ), \
	dim3( U2_NT ), ldspad, st, P )
		if( io == 6 )
		{
			U2_RAW( 6, 124 );
		}
		else
		if( io == 7 )
		{
			U2_RAW( 7, 224 );
		}
		else
		if( io == 4 )
		{
			switch( srck )
			{
				case 13: U2_RAW( 4, 13 ); break;
				case 14: U2_RAW( 4, 14 ); break;
				case 23: U2_RAW( 4, 23 ); break;
				default: U2_RAW( 4, 24 ); break;
			}
		}
		else
		{
			switch( srck )
			{
				case 13: U2_RAW( 5, 13 ); break;
				case 14: U2_RAW( 5, 14 ); break;
				case 23: U2_RAW( 5, 23 ); break;
				default: U2_RAW( 5, 24 ); break;
			}
		}
#undef U2_RAW
	}
	else
	if( io != 0 )
	{
		switch( io )
		{
			case 1: hipLaunchKernelGGL(( k_up2< U2_RB == 8, U2_RB == 8 ? 1 : 0 > ),
				dim3( items ), dim3( U2_NT ), ldspad, st, P ); break;
			case 2: hipLaunchKernelGGL(( k_up2< U2_RB == 8, U2_RB == 8 ? 2 : 0 > ),
				dim3( items ), dim3( U2_NT ), ldspad, st, P ); break;
			case 3: hipLaunchKernelGGL(( k_up2< U2_RB == 8, U2_RB == 8 ? 3 : 0 > ),
				dim3( items ), dim3( U2_NT ), ldspad, st, P ); break;
			case 4: hipLaunchKernelGGL(( k_up2< U2_RB == 8, U2_RB == 8 ? 4 : 0 > ),
				dim3( items ), dim3( U2_NT ), ldspad, st, P ); break;
			case 6: hipLaunchKernelGGL(( k_up2< U2_RB == 8, U2_RB == 8 ? 6 : 0 > ),
				dim3( items ), dim3( U2_NT ), ldspad, st, P ); break;
			case 7: hipLaunchKernelGGL(( k_up2< U2_RB == 8, U2_RB == 8 ? 7 : 0 > ),
				dim3( items ), dim3( U2_NT ), ldspad, st, P ); break;
			default: hipLaunchKernelGGL(( k_up2< U2_RB == 8, U2_RB == 8 ? 5 : 0 > ),
				dim3( items ), dim3( U2_NT ), ldspad, st, P ); break;
		}
	}
	else
	if( up2_vt( p, D ))
	{
		hipLaunchKernelGGL(( k_up2< U2_RB == 8, 0 > ), dim3( items ), dim3( U2_NT ),
			ldspad, st, P );
	}
	else
	{
		hipLaunchKernelGGL(( k_up2< false, 0 > ), dim3( items ), dim3( U2_NT ),
			ldspad, st, P );
	}
	AVIRHIP_HIPCHECK( hipGetLastError() );
#ifdef U2_DBG
	if( ++dclk_calls == 60 && items <= 8192 )
	{
		// in-kernel clocks of a launch in the middle of a timing loop
		std::vector< unsigned long long > h( items * 4 );
		(void) hipStreamSynchronize( st );
		(void) hipMemcpy( h.data(), dclk, items * 32, hipMemcpyDeviceToHost );
		double sc = 0.0, sw = 0.0, mx = 0.0;
		unsigned long long t0 = ~0ULL, t1 = 0;

		for( int i = 0; i < items; i++ )
		{
			const double w = (double) ( h[ i * 4 + 2 ] - h[ i * 4 + 1 ]);
			sc += (double) h[ i * 4 ];
			sw += w;
			mx = std::max( mx, w );
			t0 = std::min( t0, h[ i * 4 + 1 ]);
			t1 = std::max( t1, h[ i * 4 + 2 ]);
		}

		fprintf( stderr, "k_up2 clocks: mean item %.0f shader cycles, %.2f us "
			"(max %.2f us, first start to last end %.2f us) => %.3f GHz\n",
			sc / items, sw / items / 100.0, mx / 100.0,
			(double) ( t1 - t0 ) / 100.0, sc / sw * 0.1 );

		const char* dump = getenv( "AVIRHIP_UP2_CLKDUMP" );

		if( dump != nullptr )
		{
			FILE* f = fopen( dump, "w" );

			for( int i = 0; f != nullptr && i < items; i++ )
			{
				fprintf( f, "%d %llu %llu %llu %llx\n", i, h[ i * 4 ],
					h[ i * 4 + 1 ] - t0, h[ i * 4 + 2 ] - t0, h[ i * 4 + 3 ]);
			}

			if( f != nullptr ) fclose( f );
		}
	}
#endif
	return( AVIRHIP_OK );
}

} // namespace avirhip
