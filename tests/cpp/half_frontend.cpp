// A program written against the reference's API with half ("_Float16")
// pixels: compile-and-link check of the element type maps of the drop-in
// front ends (include/avir_hip/avir.h, lancir.h). Built by
// tests/test_half_table.py; running it needs a gfx950 device.
#include "avir.h"
#include "lancir.h"
#include <stdio.h>
#include <vector>

#ifndef __FLT16_MANT_DIG__
#error "this compiler has no _Float16"
#endif

int main()
{
	const int sw = 64, sh = 48, nw = 128, nh = 96;
	std::vector< _Float16 > src( (size_t) sw * sh * 4 );
	std::vector< _Float16 > dst( (size_t) nw * nh * 4 );
	std::vector< float > dstf( (size_t) nw * nh * 4 );
	std::vector< uint8_t > dst8( (size_t) nw * nh * 4 );

	for( size_t i = 0; i < src.size(); i++ )
	{
		src[ i ] = (_Float16) ( (float) ( i % 251 ) / 251.0f );
	}

	avir :: CImageResizer<> ir( 8 );
	ir.resizeImage( src.data(), sw, sh, 0, dst.data(), nw, nh, 4, 0.0 );
	ir.resizeImage( src.data(), sw, sh, 0, dstf.data(), nw, nh, 4, 0.0 );
	ir.resizeImage( src.data(), sw, sh, 0, dst8.data(), nw, nh, 4, 0.0 );

	avir :: CLancIR lr;
	const int rc = lr.resizeImage( src.data(), sw, sh, dst.data(), nw, nh, 4 );

	printf( "rc=%d %g\n", rc, (double) (float) dst[ 0 ]);
	return( 0 );
}
