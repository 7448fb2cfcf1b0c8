// A program written against the reference's API with bfloat16 ("__bf16")
// pixels: compile-and-link check of the element type maps of the drop-in
// front ends (include/avir_hip/avir.h, lancir.h). Built by
// tests/test_bf16_table.py; running it needs a gfx950 device.
#include "avir.h"
#include "lancir.h"
#include <stdio.h>
#include <string.h>
#include <vector>

#ifndef AVIRHIP_HAS_BF16
#error "this compiler has no __bf16"
#endif

// (storage only: the bits of a float's upper half, no arithmetic on __bf16)
static __bf16 bf16_of( const float v )
{
	uint32_t u;
	memcpy( &u, &v, 4 );
	const uint16_t h = (uint16_t) (( u + 0x7fffu + (( u >> 16 ) & 1u )) >> 16 );
	__bf16 r;
	memcpy( &r, &h, 2 );
	return( r );
}

static float float_of( const __bf16 v )
{
	uint16_t h;
	memcpy( &h, &v, 2 );
	const uint32_t u = (uint32_t) h << 16;
	float r;
	memcpy( &r, &u, 4 );
	return( r );
}

int main()
{
	const int sw = 64, sh = 48, nw = 128, nh = 96;
	std::vector< __bf16 > src( (size_t) sw * sh * 4 );
	std::vector< __bf16 > dst( (size_t) nw * nh * 4 );
	std::vector< float > dstf( (size_t) nw * nh * 4 );
	std::vector< uint8_t > dst8( (size_t) nw * nh * 4 );

	for( size_t i = 0; i < src.size(); i++ )
	{
		src[ i ] = bf16_of( (float) ( i % 251 ) / 251.0f );
	}

	avir :: CImageResizer<> ir( 8 );
	ir.resizeImage( src.data(), sw, sh, 0, dst.data(), nw, nh, 4, 0.0 );
	ir.resizeImage( src.data(), sw, sh, 0, dstf.data(), nw, nh, 4, 0.0 );
	ir.resizeImage( src.data(), sw, sh, 0, dst8.data(), nw, nh, 4, 0.0 );

	avir :: CLancIR lr;
	const int rc = lr.resizeImage( src.data(), sw, sh, dst.data(), nw, nh, 4 );

	printf( "rc=%d %g\n", rc, (double) float_of( dst[ 0 ]));
	return( 0 );
}
