// dnsrgb_dev.h -- the sRGB gamma stages of k_dnfh's uint8 sides (dnf.hip):
// the expressions of generic.hip's pack pass and output stage, restated for
// another translation unit under the same -ffp-contract=off build, and the
// parameters that travel with such a call.
//   loader   a colour channel v of a uint8 RGBA pixel becomes tbl[ v ] (the
//            plan's d_srgb_tbl), the alpha channel (float) v * gm
//            (k_pack_gamma_px< uint8_t, 4 >)
//   store    the byte is the number of thresholds thr[ k ] <= v, found with
//            k_epilogue_gamma_thr's eight compares over the colour half or the
//            alpha half of the plan's d_gthr; outside |v| <= 16 its direct
//            expression decides (ds_direct_byte)
#ifndef AVIRHIP_DNSRGB_DEV_H
#define AVIRHIP_DNSRGB_DEV_H

#include "plan.h"

namespace avirhip {

// pow24i_sRGB, avir.h:187-198 (generic.hip: srgb_pow24i)
__device__ __forceinline__ double ds_pow24i( const double x )
{
	const double sx = sqrt( x );
	const double ssx = sqrt( sx );
	const double sssx = sqrt( ssx );

	return( 0.000213364515060263 + 0.0149409239419218 * x +
		0.433973412731747 * sx + ssx * ( 0.659628181609715 * sssx -
		0.0380957908841466 - 0.0706476137208521 * sx ));
}

// convertLin2SRGB< float >, avir.h:301-312 (generic.hip: lin_to_srgb)
__device__ __forceinline__ float ds_lin_to_srgb( const float s )
{
	const float a = 0.055f;

	if( s <= 0.0031308f )
	{
		return( 12.92f * s );
	}

	return(( 1.0f + a ) * (float) ds_pow24i( (double) s ) - a );
}

// avir::round, avir.h:130-135 (generic.hip: avir_round)
__device__ __forceinline__ float ds_round( const float d )
{
	return( d < 0.0f ? -(float) avirhip_x86_cvtt( 0.5f - d ) :
		(float) avirhip_x86_cvtt( d + 0.5f ));
}

// the byte of a value outside the range the thresholds were searched in:
// k_epilogue_gamma_thr's direct branch, its x86 out-of-range behaviour included
__device__ __forceinline__ int ds_direct_byte( const float v, const bool alpha,
	const DnGamma& G )
{
	float d = ( alpha ? v * G.ogm : ds_lin_to_srgb( v ) * G.ogm );
	d = ( G.use_tr ? ds_round( d * G.tr_muli ) * G.tr_mul : ds_round( d ));
	d = ( d < 0.0f ? 0.0f : ( d > G.pk_out ? G.pk_out : d ));
	return( (int) (unsigned char) d );
}

// a table of N floats in LDS; only the kernels that call it hold one
template< int N >
__device__ __forceinline__ float* ds_table()
{
	__shared__ float t[ N ];
	return( t );
}

} // namespace avirhip

#endif
