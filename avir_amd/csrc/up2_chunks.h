// up2_chunks.h -- how k_up2 (up2.hip) cuts a strip into chunks of source rows.
// Plain C++ (constexpr functions only): the kernel, up2_run and a host-only
// test program (tests/test_up2_chunks.py) all include this one statement of
// the rule.
//
// A chunk of h source rows costs ceil(( h + 18 ) / U2_RB ) marching steps (6
// rows of preload + 12 of warm-up), so heights of the form U2_RB * k - 18
// waste nothing. A strip is cut into chunks of TWO such heights one step
// apart, the long ones first:
//     chunk c < nlong :  cq + U2_RB rows        chunk c >= nlong :  cq rows
//     first row of chunk c = c * cq + U2_RB * min( c, nlong )
// and the frame's end clips the last chunk. With one height (nlong = 0) the
// rows left over made a short last chunk per strip, and with every work item
// resident at once nothing fills the slot such a chunk frees early; two
// heights deal the same marching steps out evenly.

#ifndef AVIRHIP_UP2_CHUNKS_H
#define AVIRHIP_UP2_CHUNKS_H

#ifndef U2_RB
#define U2_RB 8 // source rows per marching step
#endif

namespace avirhip {

// (first source row of chunk c)
constexpr int up2_chunk_first( const int c, const int cq, const int nlong )
{
	return( c * cq + U2_RB * ( c < nlong ? c : nlong ));
}

// (source rows of chunk c, before the frame's end clips it)
constexpr int up2_chunk_rows( const int c, const int cq, const int nlong )
{
	return( c < nlong ? cq + U2_RB : cq );
}

// U2_TAIL: what the transposed form (k_up2< true >) does in a chunk's last
// marching step, from the fourth step on -- 2: no dead vertical sums and no
// woven H1, 1: no woven H1 only, 0: the steady body (for A/B builds).
#ifndef U2_TAIL
#define U2_TAIL 2
#endif

// Which running sums want tap t's product of a row (up2_vt.inl), by the mode
// of the row's marching step. Row g of the ring, row rr of its step, carries
// C2[ m ]; the product goes to even( m+3-t ) and to odd( m-9+t ).
//   1 steady: both, always.
//   2 the chunk's first 24 rows (row j = g of the chunk): sums of rows before
//     the chunk are left alone -- even for t <= j - 6, odd for t >= 18 - j.
//   3 the chunk's last step: its last row carries m = qe + 8, where 2 * qe is
//     the first output row after the step, so row rr carries m = qe + 1 + rr.
//     Sums of the rows from 2 * qe on are left alone: even( m+3-t ) lies below
//     qe for t >= rr + 5, odd( m-9+t ) for t <= 7 - rr. Per thread that leaves
//     64 of the 192 adds and 60 of the 96 multiplies of a step (a product is
//     computed iff one of its sums wants it). A chunk that the frame's end
//     clips ends before 2 * qe: the rule keeps more than it needs, never less.
constexpr bool up2_want_even( const int mode, const int g, const int rr,
	const int t )
{
	return( mode == 2 ? t <= g - 6 :
		( mode == 3 && U2_TAIL >= 2 ? t >= rr + 5 : true ));
}

constexpr bool up2_want_odd( const int mode, const int g, const int rr,
	const int t )
{
	return( mode == 2 ? t >= 18 - g :
		( mode == 3 && U2_TAIL >= 2 ? t <= 7 - rr : true ));
}

// (the chunk that holds source row q)
constexpr int up2_chunk_of( const int q, const int cq, const int nlong )
{
	return( q < nlong * ( cq + U2_RB ) ? q / ( cq + U2_RB ) :
		nlong + ( q - nlong * ( cq + U2_RB )) / cq );
}

struct Up2Split
{
	int n;     // chunks that cover the band
	int cq;    // rows of a short chunk, U2_RB * k - 18
	int nlong; // leading chunks of cq + U2_RB rows
};

#define UP2_KMIN 10 // marching steps of the shortest chunk the choice makes
#define UP2_KMAX 64 // ... of the tallest
#define UP2_NCU 256 // compute units the work items are dealt over
#define UP2_RES 8   // workgroups of k_up2 resident on one

// `rows` source rows in n chunks: S = ceil(( rows + 18 n ) / U2_RB ) marching
// steps dealt as evenly as they go, S % n chunks get one more than the rest.
// The rows they hold exceed `rows` by less than U2_RB, so the clipped last
// chunk still needs all of its steps. kmin: the fewest steps a chunk may have
// (>= 4: the kernel's first 24 rows are one code path, and a chunk has to be
// taller than the up to 7 rows the last one is clipped by); n = 0 if n chunks
// would be shorter.
constexpr Up2Split up2_split_n( const int rows, const int n, const int kmin )
{
	const int S = ( rows + 18 * n + U2_RB - 1 ) / U2_RB;
	const int k = ( n == 1 && S < kmin ? kmin : S / n );

	if( k < kmin )
	{
		return( Up2Split{ 0, 0, 0 });
	}

	return( Up2Split{ n, U2_RB * k - 18, ( n == 1 ? 0 : S - n * k )});
}

// The long chunks the most loaded CU can hold. Work items are strip-major
// and an XCD hands its workgroups to its 32 CUs in turn (the per-CU dumps of
// profiles/up2_chunks/ show it), so a CU's m items are 32 items apart: chunks
// c, c + 32, c + 64 ... modulo n. With n = 16 they are ONE chunk, all long or
// all short; with n = 17 they are m different ones.
constexpr int up2_split_longs( const Up2Split s, const int m )
{
	int worst = 0;

	for( int c = 0; c < s.n; c++ )
	{
		int l = 0;

		for( int t = 0; t < m; t++ )
		{
			l += (( c + 32 * t ) % s.n < s.nlong );
		}

		worst = ( l > worst ? l : worst );
	}

	return( worst );
}

// Step-times of a launch of nstrips strips cut by `s`. The kernel is VALU-bound
// and a CU shares its VALUs among its resident workgroups, so a launch whose
// items are all resident at once ends when the most loaded CU does: that CU
// holds m = ceil( items / 256 ) items, up2_split_longs of them long, and
// thr[ m ] is the measured VALU throughput of a CU that runs m workgroups.
// Launches of more than 8 x 256 items run in partial rounds and measured 7-8 %
// worse than their step count.
constexpr double up2_split_cost( const Up2Split s, const int nstrips )
{
	constexpr double thr[ UP2_RES + 1 ] = { 1.0, 0.3, 0.57, 0.8, 0.9, 0.9,
		0.9, 0.97, 1.0 };
	const int k = ( s.cq + 18 ) / U2_RB;
	const long items = (long) s.n * nstrips;
	const int m = (int) (( items + UP2_NCU - 1 ) / UP2_NCU );

	return( m <= UP2_RES ?
		(double) ( m * k + up2_split_longs( s, m )) / thr[ m ] :
		(double) nstrips * ( s.n * k + s.nlong ) / UP2_NCU * 1.08 );
}

// The split of a band of `rows` source rows and nstrips strips: the chunk
// count of the least cost, the fewest chunks among equals. Few tall chunks
// waste little warm-up work, many short ones balance and fill the CUs. A band
// that fits the shortest chunk stays one chunk.
constexpr Up2Split up2_split_choose( const int rows, const int nstrips )
{
	Up2Split best = up2_split_n( rows, 1, UP2_KMIN );
	double bc = -1.0;

	for( int n = 1; ; n++ )
	{
		const Up2Split s = up2_split_n( rows, n, UP2_KMIN );

		if( s.n == 0 )
		{
			break;
		}

		if(( s.cq + 18 ) / U2_RB + ( s.nlong > 0 ) > UP2_KMAX )
		{
			continue;
		}

		const double c = up2_split_cost( s, nstrips );

		if( bc < 0.0 || c < bc )
		{
			bc = c;
			best = s;
		}
	}

	return( best );
}

} // namespace avirhip

#endif
