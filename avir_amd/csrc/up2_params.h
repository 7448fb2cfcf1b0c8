// up2_params.h -- k_up2's kernel parameters (up2.hip), and what up2_run asks
// about a plan with sRGB gamma, whose kinds of the kernel (IO 8 / 9, SRC 313 /
// 314) take the gamma stages' tables and constants behind them.
#ifndef AVIRHIP_UP2_PARAMS_H
#define AVIRHIP_UP2_PARAMS_H

#include "plan.h"
#include "dnsrgb_dev.h"
#include <math.h>
#include <type_traits>

// Floats of the de-linearising stage's thresholds that the IO 8 / 9 kinds copy
// into LDS: 512, the colour half and the alpha half (2 KB); 256, the colour
// half alone, alpha by the stage's direct expression (1 KB: the residency
// experiment of `make thr1k`, NOTEBOOK section 34)
#ifndef U2_GTHR
#define U2_GTHR 512
#endif

namespace avirhip {

struct Up2Params
{
	const float* src; long src_ss; int sw, sh;
	int rmin, rmax; // source rows that exist behind `src` (a window: plan.h)
	float* dst; long dst_ss; int dst_row0; int nw, nh;
	int srow_lo, srow_hi;
	int nstrips, chunk0, nchunks;
	int cq, nlong; // source rows (output row pairs) per chunk: the first nlong
		// chunks of a strip hold cq + U2_RB, the others cq (up2_chunks.h)
	// IO != 0: the caller's image instead of dst -- uint8 / uint16 (the output
	// stage of dither(), avir.h:4392-4419, without bit-depth truncation) or
	// float pixels of 1-3 channels; ibase = the band's first row
	void* ibase; int istride_b; int ich;
#ifdef U2_DBG
	int dbg; // timing ablations (debug build only)
	unsigned long long* clk; // [items][4]: shader cycles, start, end (100 MHz ticks), hw id
#endif
	const float* coef; // device: the taps, horizontal axis first, packed
		// (2 x 32 floats) and paired (2 x 64 from U2_PAIRED): see Taps
};

// The same fields at the same kernel-argument offsets, and behind them the two
// stages' tables and constants. No other kind sees them.
struct Up2GParams : Up2Params
{
	DnGamma G;
};

template< int IO >
constexpr bool up2_gamma_out = ( IO == 8 || IO == 9 );

// the parameter type of k_up2< VT, IO, SRC >
template< int IO >
using Up2PT = std::conditional_t< up2_gamma_out< IO >, Up2GParams, Up2Params >;

// The gain of one axis' two filters: the product of their taps' absolute sums.
// The product of both axes' bounds every sum of samples within [-1, 1]; IO 9
// wants it below 16, the range the thresholds were searched in (up2_prepare
// asks for 15: the headroom covers the float sums' rounding many times over).
static double up2_axis_gain( const float* f, const float* fe, const float* fo )
{
	double g = fabs( (double) f[ 0 ]), e = 0.0, o = 0.0;

	for( int i = 1; i < 4; i++ )
	{
		g += 2.0 * fabs( (double) f[ i ]);
	}

	for( int t = 0; t < 12; t++ )
	{
		e += fabs( (double) fe[ t ]);
		o += fabs( (double) fo[ t ]);
	}

	return( g * ( e > o ? e : o ));
}

// Whether an integer image may be read where it lies, by `io`: results of
// integer sources (4 / 5) of a uint8 / uint16 image; with gamma the
// de-linearised result of one (9) of a uint8 image, through the plan's table.
static bool up2_int_raw_ok( const avirhip_plan* p, const int io )
{
	if( p -> gamma )
	{
		return( io == 9 && p -> in_type == AVIRHIP_U8 &&
			p -> d_srgb_tbl != nullptr );
	}

	return(( io == 4 || io == 5 ) && ( p -> in_type == AVIRHIP_U8 ||
		p -> in_type == AVIRHIP_U16 ));
}

// The stages' constants: launch_pack_gamma's and launch_epilogue's for uint8
static void up2_gamma_params( const avirhip_plan* p, DnGamma& G )
{
	G.tbl = p -> d_srgb_tbl;
	G.thr = p -> d_gthr;
	G.alpha_index = p -> alpha_index;
	G.use_tr = ( p -> tr_mul != 1.0 );
	G.gm = (float) ( 1.0 / 255.0 );
	G.ogm = 255.0f;
	G.tr_mul = (float) p -> tr_mul;
	G.tr_muli = (float) ( 1.0 / p -> tr_mul );
	G.pk_out = (float) p -> pk_out;
}

} // namespace avirhip

#endif
