// generic64.hip -- the double pipeline: avir::CImageResizer< fpclass_def< double > >
// (avir.h:4553-4560). Every table of such a plan is built in double by the
// planner's double instantiation (planner_avir.inl: the reference stores,
// accumulates and reads back its filters in `fptype`, so the double tables are
// not the float ones widened), and every pass computes in double: one kernel
// launch per lowered op with the intermediates in HBM -- generic.hip's per-op
// kernels and api.cpp's driver (run_generic) in their double instantiation,
// between this file's own pack pass and output stage; the reference's own example of this class is an accuracy option,
// not a speed one, and no fast path exists for it here either.
//
// Arithmetic contract (compiled -ffp-contract=off): separate v_mul_f64 /
// v_add_f64 in the reference's order, sums started from +0.0 -- bit-identical
// to the reference built the same way (tests: oracle/_ref, variant 4).

#include "plan.h"
#include "f64_dev.h"
#include <string.h>
#include <stdint.h>
#include <type_traits>

namespace avirhip {

namespace {

// pow24_sRGB / pow24i_sRGB, avir.h:161-196: evaluated in double whatever T is
__device__ __forceinline__ double pow24_64( const double x )
{
	const double x2 = x * x;
	const double x3 = x2 * x;
	const double x4 = x2 * x2;

	return( 0.0985766365536824 + 0.839474952656502 * x2 +
		0.363287814061725 * x3 - 0.0125559718896615 /
		( 0.12758338921578 + 0.290283465468235 * x ) -
		0.231757513261358 * x - 0.0395365717969074 * x4 );
}

__device__ __forceinline__ double pow24i_64( const double x )
{
	const double sx = sqrt( x );
	const double ssx = sqrt( sx );
	const double sssx = sqrt( ssx );

	return( 0.000213364515060263 + 0.0149409239419218 * x +
		0.433973412731747 * sx + ssx * ( 0.659628181609715 * sssx -
		0.0380957908841466 - 0.0706476137208521 * sx ));
}

// packScanline, avir.h:2777-2930: the (fptype) cast per element, zero padding
// up to `ech` channels; with gamma the colour channels are linearised
// (convertSRGB2Lin< double, Tin >, avir.h:207-291: uint8 through the table of
// float literals), the alpha channel only scaled by InGammaMult.
template< typename Tin >
__global__ void __launch_bounds__( 256 ) k_pack64( const Tin* src, double* dst,
	int row_elems, int h, long src_stride, int ch, int ech, int gamma,
	int alpha_index, double gm, const float* tbl )
{
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	const int y = blockIdx.y;

	if( x >= row_elems || y >= h )
	{
		return;
	}

	const int px = x / ech;
	const int c = x - px * ech;
	double r = 0.0;

	if( c < ch )
	{
		const Tin v = src[ (long) y * src_stride + px * ch + c ];

		if( !gamma )
		{
			r = (double) v;
		}
		else
		if( c == alpha_index )
		{
			r = (double) v * gm;
		}
		else
		if( sizeof( Tin ) == 1 )
		{
			r = (double) tbl[ (int) v ];
		}
		else
		{
			const double s = (double) v * gm;
			const double a = 0.055;
			r = ( s <= 0.04045 ? s / 12.92 : pow24_64(( s + a ) / ( 1.0 + a )));
		}
	}

	dst[ (long) y * row_elems + x ] = r;
}

// applySRGBGamma (avir.h:2982-3068), CImageResizerDithererDefINL< double >::
// dither (avir.h:4392-4419) for integer outputs, unpackScanline's (Tout) cast
// (avir.h:3155-3215); `res` holds ech >= ch channels per pixel.
template< typename Tout >
__global__ void __launch_bounds__( 256 ) k_epilogue64( const double* res,
	Tout* dst, long n, int use_tr, double tr_mul, double tr_muli, double pk_out,
	int gamma, int ch, int ech, int alpha_index, double ogm )
{
	const long i = (long) blockIdx.x * blockDim.x + threadIdx.x;

	if( i >= n )
	{
		return;
	}

	const long px = i / ch;
	const int c = (int) ( i - px * ch );
	double v = res[ px * ech + c ];

	if( gamma )
	{
		if( c == alpha_index )
		{
			v = v * ogm;
		}
		else
		{
			const double a = 0.055;
			v = ( v <= 0.0031308 ? 12.92 * v : ( 1.0 + a ) * pow24i_64( v ) - a ) *
				ogm;
		}
	}

	dst[ i ] = out_stage64< Tout >( use_tr, tr_mul, tr_muli, pk_out, v );
}

int dalloc( avirhip_plan* p, const size_t bytes, double** out )
{
	void* q = nullptr;
	AVIRHIP_HIPCHECK( hipMalloc( &q, bytes ));
	p -> allocs.push_back( q );
	p -> alloc_bytes += bytes;
	*out = (double*) q;
	return( AVIRHIP_OK );
}

} // namespace

// Output rows [row0, row1) of a double-pipeline plan: pack (unless the source
// is the double image the first pass can read as it is), the horizontal ops
// over the source rows the band's vertical windows read, the vertical ops,
// then the output stage -- or, for double output, the vertical pass' in-place
// result (avir.h:4956-4979: IsOutFloat && sizeof( fptype ) == sizeof( Tout );
// float output goes through unpackScanline and is de-linearised with gamma).
int exec_f64( avirhip_plan* p, const void* src, void* dst, int row0, int row1,
	hipStream_t st )
{
	if( row1 <= row0 )
	{
		return( AVIRHIP_OK );
	}

	int rc;
	const int ch = p -> ch; // (== io_ch: no RGBA padding here)
	// the tiled two-pass kernels (tile64.hip) run every plan without a filtered
	// upsample unless path 1 is forced: their H pass reads the caller's image
	// itself and their V pass stores through the output stage, so without gamma
	// neither the double copy of the source nor the double result exists
	const int xpath = ( p -> path != 0 ? p -> path : p -> auto_path );
	const bool tiled = ( xpath != 1 && tile64_ok( p ));
	const bool need_pack = ( tiled ? p -> gamma != 0 :
		( p -> gamma || p -> in_type != AVIRHIP_F64 ));
	const bool direct = ( p -> out_type == AVIRHIP_F64 ||
		( tiled && !p -> gamma ));

	if( need_pack && p -> packed64 == nullptr &&
		( rc = dalloc( p, (size_t) p -> src_w * p -> src_h * ch *
		sizeof( double ), &p -> packed64 )) != 0 ) return( rc );

	if( !direct && p -> resbuf64 == nullptr &&
		( rc = dalloc( p, (size_t) p -> new_w * p -> new_h * ch *
		sizeof( double ), &p -> resbuf64 )) != 0 ) return( rc );

	if( !tiled && ( rc = ensure_generic_scratch< double >( p )) != 0 )
		return( rc );

	const VRanges R = v_ranges( p -> v, row0, row1 );
	const int ya = R.ya, yb = R.yb; // FltBuf rows needed

	const double* fsrc = (const double*) src;
	long sstride = p -> src_stride;

	if( need_pack )
	{
		const int re = p -> src_w * ch;
		const int rows = yb - ya + 1;
		const dim3 grd(( re + 255 ) / 256, rows );
		// InGammaMult, avir.h:4744-4754
		const double gm = ( p -> in_type == AVIRHIP_U8 ? 1.0 / 255.0 :
			( p -> in_type == AVIRHIP_U16 ? 1.0 / 65535.0 : 1.0 ));

		double* const pd = p -> packed64 + (size_t) ya * re;

#define PK( T ) hipLaunchKernelGGL( k_pack64< T >, grd, dim3( 256 ), 0, st, \
		(const T*) src + (size_t) ya * p -> src_stride, pd, re, rows, \
		(long) p -> src_stride, ch, ch, p -> gamma, p -> alpha_index, gm, \
		p -> d_srgb_tbl )

		switch( p -> in_type )
		{
			case AVIRHIP_U8: PK( uint8_t ); break;
			case AVIRHIP_U16: PK( uint16_t ); break;
			case AVIRHIP_F32: PK( float ); break;
			default: PK( double ); break;
		}

#undef PK
		AVIRHIP_HIPCHECK( hipGetLastError() );
		fsrc = p -> packed64;
		sstride = re;
	}

	if( tiled )
	{
		void* const tdst = ( direct ? dst : (void*) p -> resbuf64 );

		rc = tile64_run( p, fsrc, ( need_pack ? AVIRHIP_F64 : p -> in_type ),
			sstride, tdst, ( p -> gamma && p -> out_type != AVIRHIP_F64 ?
			AVIRHIP_F64 : p -> out_type ), (long) p -> new_w * ch, row0, row1,
			ya, yb, st );

		if( rc != 0 || direct )
		{
			return( rc );
		}
	}

	double* const fdst = ( direct ? (double*) dst : p -> resbuf64 );

	if( !tiled && ( rc = run_generic< double >( p, fsrc, sstride, fdst, row0,
		row1, st )) != 0 ) return( rc );

	if( direct )
	{
		return( AVIRHIP_OK );
	}

	const long n = (long) ( row1 - row0 ) * p -> new_w * ch;
	const dim3 grd( (unsigned) (( n + 255 ) / 256 ));
	const int use_tr = ( p -> tr_mul != 1.0 );
	// OutGammaMult, avir.h:4756-4763
	const double ogm = ( p -> out_type == AVIRHIP_U8 ? 255.0 :
		( p -> out_type == AVIRHIP_U16 ? 65535.0 : 1.0 ));

#define EP( T ) hipLaunchKernelGGL( k_epilogue64< T >, grd, dim3( 256 ), 0, \
	st, (const double*) fdst, (T*) dst, n, use_tr, p -> tr_mul, \
	1.0 / p -> tr_mul, p -> pk_out, p -> gamma, ch, ch, p -> alpha_index, ogm )

	switch( p -> out_type )
	{
		case AVIRHIP_U8: EP( uint8_t ); break;
		case AVIRHIP_U16: EP( uint16_t ); break;
		default: EP( float ); break;
	}

#undef EP
	AVIRHIP_HIPCHECK( hipGetLastError() );
	return( AVIRHIP_OK );
}

} // namespace avirhip
