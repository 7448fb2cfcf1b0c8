// Prints what avir_amd/csrc/up2_chunks.h makes of every band height
// (tests/test_up2_chunks.py reads it): one line per case,
//   rows nstrips n cq nlong inverse_mismatches first[0] ... first[n]
// with first[] from up2_chunk_first and the mismatch count from walking every
// source row through up2_chunk_of.
#include <stdio.h>
#include <stdlib.h>
#include "up2_chunks.h"

using namespace avirhip;

// (the choice is usable in constant expressions: cfg3)
static_assert( up2_split_choose( 2160, 120 ).n >= 1, "constexpr" );

int main( int argc, char** argv )
{
	const int maxrows = ( argc > 1 ? atoi( argv[ 1 ]) : 4400 );

	for( int a = 2; a < argc || a == 2; a++ )
	{
		const int ns = ( a < argc ? atoi( argv[ a ]) : 120 );

		for( int rows = 1; rows <= maxrows; rows++ )
		{
			const Up2Split s = up2_split_choose( rows, ns );
			int bad = 0;
			int c = 0;

			for( int q = 0; q < rows; q++ )
			{
				while( up2_chunk_first( c, s.cq, s.nlong ) +
					up2_chunk_rows( c, s.cq, s.nlong ) <= q )
				{
					c++;
				}

				bad += ( up2_chunk_of( q, s.cq, s.nlong ) != c ||
					q < up2_chunk_first( c, s.cq, s.nlong ));
			}

			printf( "%d %d %d %d %d %d", rows, ns, s.n, s.cq, s.nlong, bad );

			for( int i = 0; i <= s.n; i++ )
			{
				printf( " %d", up2_chunk_first( i, s.cq, s.nlong ));
			}

			printf( "\n" );
		}
	}

	return( 0 );
}
