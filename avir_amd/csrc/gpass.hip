// gpass.hip -- pass kernels for general (non-2x) ratios: ONE AXIS PER LAUNCH,
// autonomous wavefronts, every dynamically indexed window in LDS rings.
//
// A lowered axis (plan.h) of the common plans is one of
//   PRE   FIR7 then GATHER     upsizing: correction filter, then the 12-tap
//                              interpolation over the zero-stuffed view
//                              (doFilter 3748 + doUpsample 3260 + doResize2 4114)
//   POST  GATHER then FIR7     downsizing: NT-tap resize, then the correction
//                              filter (doResize 3884 / doResize2 + doFilter)
//   NONE  GATHER               LANCIR's N-tap dot products (lancir.h:2466-2544)
// with a position table (first input index per output) and one coefficient row
// per output (AVIR) or per fractional phase (LANCIR). The tiled interpreter of
// fused.hip runs any chain but keeps whole 2-D tiles in LDS: two workgroups
// per CU, phases separated by barriers, half of its wave-cycles parked
// (profiles/r02_tile). Here a wavefront owns a strip and never synchronises
// with another wave:
//
//   k_gv  vertical pass. Lane = whole pixel of a 64-pixel strip (half pixel /
//         32-pixel strips for images narrower than 49 pixels): a row is one
//         contiguous 1-KiB segment. Source rows arrive by LDS-DMA in a landing
//         queue, read a step ahead of their use; the FIR7 window and -- for
//         the tap counts that occur -- the gather window live in registers
//         (the step loop is unrolled to the window length, ring slots are
//         compile-time); coefficient rows are staged in LDS per chunk and read
//         as broadcasts one output ahead.
//   k_gh  horizontal pass. Lane = whole output pixel (16 B) of a strip of up
//         to 64 outputs; its coefficient row stays in registers while the wave
//         walks down its rows; the row's source segment arrives by LDS-DMA
//         three rows ahead.
//   k_sacc (sacc.hip) takes the downsizing axes (k >= 2) of integer / narrow
//         sources: streaming accumulation instead of a gather window.
//
// Arithmetic contract (bit-exact): mul and add separate (-ffp-contract=off),
// AVIR sums start from +0.0f and take their taps in ascending order, the FIR
// is f0*c + sum f_i*(right_i + left_i); LANCIR accumulates even and odd taps
// separately from bare first products and adds the two sums at the end.

#include "gpass_dev.h"
#include <algorithm>
#include <math.h>
#include <type_traits>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>

namespace avirhip {

// ---------------------------------------------------------------------
// horizontal pass
// ---------------------------------------------------------------------

#ifndef GH_NB
#define GH_NB 4 // source row buffers: rows r .. r + 3 are in LDS or in flight
#endif

// SRC: 0 float RGBA by LDS-DMA; 1 uint8, 2 uint16, 3 float pixels of raw_ch
// channels, read as they are (packScanline's cast and zero padding,
// avir.h:2777-2840, in the loader: no float copy of the source): a lane loads
// its pixel of each 64-pixel piece a row ahead, converts and writes it into
// the row buffer after the row in hand has been computed.
template< int SRC > struct GHElem { typedef float T; };
template<> struct GHElem< 1 > { typedef unsigned char T; };
template<> struct GHElem< 2 > { typedef unsigned short T; };

// (LANCIR plans have float RGBA sources only: there the fourth parameter is the
// compile-time kind of the output stage, gp_store_lancir_row)
template< int MODE, bool LANC, int NTC, int SX >
__global__ void __launch_bounds__( 64 ) k_gh( const GHParams P )
{
	constexpr int SRC = ( LANC ? 0 : SX );
	constexpr int OUTK = ( LANC ? SX : 0 );
	extern __shared__ __attribute__(( aligned( 16 ))) char smem[];
	const GPAxis& A = P.ax;
	f4* const sbuf = (f4*) smem;                    // [GH_NB][sbuf px]
	f4* const mbuf = sbuf + GH_NB * (size_t) P.sbuf; // [mbuf px]
	float* const cfl = (float*) ( mbuf + P.mbuf );  // NTC == 0: [nt][64 lanes]
	const unsigned sbuf_lds = (unsigned) (unsigned long) (lds_char*) smem;

	const int lane = threadIdx.x;
	const int strip = blockIdx.x % P.nstrips;
	const int chunk = blockIdx.x / P.nstrips;
	const int r0 = P.row_lo + chunk * P.chunk;
	const int r1 = min( r0 + P.chunk, P.row_hi );

	if( r0 >= r1 )
	{
		return;
	}

	const int slo = P.seg[ strip * 4 ], scnt = P.seg[ strip * 4 + 1 ];
	const int mlo = P.seg[ strip * 4 + 2 ], mcnt = P.seg[ strip * 4 + 3 ];
	const int j0 = strip * P.ow;
	const int j = j0 + lane;                        // this lane's output
	const bool jok = ( lane < P.ow && j < A.out_len );
	const int nt = ( NTC > 0 ? NTC : A.nt );
	const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
		(void*) P.src, 0, 0x7fffffff, 0x00020000 );
	const int srow_b = (int) P.src_ss * 4;

	// per-lane source pixels of the DMA pieces (clamped: the extended view)
	const int slast = A.in_len - 1;

	// (the clamped columns once, not per row: four registers -- which the
	// any-tap-count variant, NTC == -1, does not have: 168 -> 172 VGPRs is three
	// waves per SIMD -> two)
	constexpr bool XB = ( NTC != -1 );
	int xb[ 4 ];
#pragma unroll
	for( int k = 0; k < 4; k++ )
	{
		xb[ k ] = ( XB ? gp_clamp( slo + k * 64 + lane, slast ) * 16 : 0 );
	}

	auto issue_row = [&]( const int r, const int buf )
	{
		const int rb = r * srow_b;
		const unsigned lb = sbuf_lds + ( buf * P.sbuf ) * 16;

		if( XB && P.nseg <= 4 )
		{
#pragma unroll
			for( int k = 0; k < 4; k++ )
			{
				if( k < P.nseg )
				{
					gp_dma( rsrc, lb + k * 1024, rb + xb[ k ]);
				}
			}
		}
		else
		for( int k = 0; k < P.nseg; k++ )
		{
			const int x = gp_clamp( slo + k * 64 + lane, slast );
			gp_dma( rsrc, lb + k * 1024, rb + x * 16 );
		}
	};

	// The gather this lane evaluates, its first input (relative to the
	// buffer it reads) and its coefficient row -- fixed for every row.
	//   PRE / NONE: gather output == final output j
	//   POST: lane l evaluates G[ mlo + l ] (the strip's outputs +- 3)
	const int g = ( MODE == GP_POST ? gp_clamp( mlo + lane, A.g_len - 1 ) :
		gp_clamp( j, A.g_len - 1 ));

	const bool gok = ( MODE == GP_POST ? lane < mcnt : jok );
	const int gs = A.start[ g ] - ( MODE == GP_PRE ? mlo : slo );
	// a compile-time tap count keeps the row in registers; any other count
	// parks it in LDS, tap-major (lane-consecutive: conflict-free reads)
	// (NTC == -1: any count up to 28, in registers too)
	float cf[ NTC > 0 ? NTC : ( NTC < 0 ? 28 : 1 )];
	{
		const float* cr = A.coef + (long) ( LANC ? A.fidx[ g ] : g ) * nt;

		if( NTC < 0 )
		{
#pragma unroll
			for( int t = 0; t < ( NTC < 0 ? 28 : 1 ); t++ )
			{
				cf[ t ] = ( t < nt ? cr[ t ] : 0.0f );
			}
		}
		else
		if( NTC > 0 )
		{
#pragma unroll
			for( int t = 0; t < ( NTC > 0 ? NTC : 1 ); t++ )
			{
				cf[ t ] = cr[ t ];
			}
		}
		else
		{
			for( int t = 0; t < nt; t++ )
			{
				cfl[ t * 64 + lane ] = cr[ t ];
			}
		}
	}

	// typed sources: the row in flight (up to four pieces, four channels)
	f4 rw[ SRC != 0 ? 4 : 1 ];

	auto t_load = [&]( const int r )
	{
#pragma unroll
		for( int k = 0; k < ( SRC != 0 ? 4 : 1 ); k++ )
		{
			if( k < P.nseg )
			{
				rw[ k ] = gp_load_raw( P.raw, SRC, P.raw_ch, (long) r * P.raw_ss +
					(long) gp_clamp( slo + k * 64 + lane, slast ) * P.raw_ch,
					P.raw_elems );
			}
		}
	};

	auto t_store = [&]( const int buf )
	{
#pragma unroll
		for( int k = 0; k < ( SRC != 0 ? 4 : 1 ); k++ )
		{
			if( k < P.nseg )
			{
				sbuf[ buf * P.sbuf + k * 64 + lane ] = rw[ k ];
			}
		}
	};

	if( SRC != 0 )
	{
		t_load( r0 );
		t_store( 0 );

		if( r0 + 1 < r1 )
		{
			t_load( r0 + 1 );
		}
	}
	else
	{
		for( int k = 0; k < GH_NB - 1 && r0 + k < r1; k++ )
		{
			issue_row( r0 + k, k );
		}
	}

	for( int r = r0; r < r1; r++ )
	{
		const int buf = ( r - r0 ) & ( GH_NB - 1 );
		const f4* const s = sbuf + buf * P.sbuf;
		GP_PRIO_LOW();

		if( SRC == 0 )
		{
			// row r + 3 goes out (into the buffer row r - 1 has left), then
			// wait for row r: only the pieces of the rows after it may be in
			// flight
			if( r + GH_NB - 1 < r1 )
			{
				issue_row( r + GH_NB - 1, ( buf + GH_NB - 1 ) & ( GH_NB - 1 ));
			}

			// (the count stands for LOADS only. The stores of the rows that left
			// meanwhile count on vmcnt too, but they do not retire in order with
			// the loads -- a store's acknowledgement can overtake an older load
			// (measured in sacc.hip's feed at the end of round 4: a count that
			// included "the stores since" let a group be used before it landed)
			// -- so they may only make this wait longer, never shorter. Rounds
			// 3-4 added them to the count here; no mismatch was ever seen, but
			// it was a race.)
			// (steady state: the count per segment count spelled out -- the
			// general count walks gp_wait_vm's 25-way ladder, ten branches a row)
			if( r1 - 1 - r >= GH_NB - 1 && P.nseg <= 4 )
			{
				if( P.nseg <= 2 )
				{
					if( P.nseg == 1 ) gp_wait_vm(( GH_NB - 1 ) * 1 );
					else gp_wait_vm(( GH_NB - 1 ) * 2 );
				}
				else
				{
					if( P.nseg == 3 ) gp_wait_vm(( GH_NB - 1 ) * 3 );
					else gp_wait_vm(( GH_NB - 1 ) * 4 );
				}
			}
			else
			{
				gp_wait_vm( min( GH_NB - 1, r1 - 1 - r ) * P.nseg );
			}
		}

		if( !LANC && MODE != GP_PRE && slo + scnt - 1 > A.view_mmax )
		{
			// zero-stuffed view of the source: its tail reads 0
			for( int x = lane; x < scnt; x += 64 )
			{
				if( slo + x > A.view_mmax )
				{
					((f4*) s )[ x ] = (f4) 0.0f;
				}
			}
		}

		if( MODE == GP_PRE )
		{
			// C[ mlo .. mlo + mcnt ) = FIR7 along x of the segment
			for( int i = lane; i < mcnt; i += 64 )
			{
				const int m = mlo + i;
				f4 c;

				if( m > A.view_mmax )
				{
					c = (f4) 0.0f;
				}
				else
				{
					const f4* q = s + ( gp_clamp( m, A.c_len - 1 ) - A.e - slo );
					c = A.f[ 0 ] * q[ 0 ];
					c = c + A.f[ 1 ] * ( q[ 1 ] + q[ -1 ]);
					c = c + A.f[ 2 ] * ( q[ 2 ] + q[ -2 ]);
					c = c + A.f[ 3 ] * ( q[ 3 ] + q[ -3 ]);
				}

				mbuf[ i ] = c;
			}
		}

		f4 o = (f4) 0.0f;

		if( gok )
		{
			const f4* const in = ( MODE == GP_PRE ? mbuf : s ) + gs;
			// a compile-time tap count: the whole window is read first (all
			// its ds_read_b128 in flight at once), then the arithmetic runs
			// -- left alone the compiler keeps two reads in flight and pays
			// the LDS latency six times per pixel
			f4 w[ NTC > 0 ? NTC : 1 ];

			if( NTC > 0 )
			{
#pragma unroll
				for( int t = 0; t < ( NTC > 0 ? NTC : 1 ); t++ )
				{
					w[ t ] = in[ t ];
				}

				__builtin_amdgcn_sched_barrier( 0 );
			}

			GP_PRIO_HIGH();
			o = gp_dot< LANC, f4, NTC >( nt,
				[&]( const int t ) { return( NTC > 0 ?
					w[ NTC > 0 ? t % ( NTC > 0 ? NTC : 1 ) : 0 ] : in[ t ]); },
				[&]( const int b ) -> f4
				{
					f4 c;

					if( NTC < 0 )
					{
						c.x = cf[ NTC < 0 ? ( 4 * b ) % 28 : 0 ];
						c.y = cf[ NTC < 0 ? ( 4 * b + 1 ) % 28 : 0 ];
						c.z = cf[ NTC < 0 ? ( 4 * b + 2 ) % 28 : 0 ];
						c.w = cf[ NTC < 0 ? ( 4 * b + 3 ) % 28 : 0 ];
					}
					else
					if( NTC > 0 )
					{
						c.x = cf[ ( 4 * b ) % ( NTC > 0 ? NTC : 1 )];
						c.y = cf[ ( 4 * b + 1 ) % ( NTC > 0 ? NTC : 1 )];
						c.z = cf[ ( 4 * b + 2 ) % ( NTC > 0 ? NTC : 1 )];
						c.w = cf[ ( 4 * b + 3 ) % ( NTC > 0 ? NTC : 1 )];
					}
					else
					{
						// (rows beyond nt hold whatever: never multiplied)
						c.x = cfl[ ( 4 * b ) * 64 + lane ];
						c.y = cfl[ ( 4 * b + 1 ) * 64 + lane ];
						c.z = cfl[ ( 4 * b + 2 ) * 64 + lane ];
						c.w = cfl[ ( 4 * b + 3 ) * 64 + lane ];
					}

					return( c );
				}, A.lanc, true );
		}

		if( MODE == GP_POST )
		{
			if( gok )
			{
				mbuf[ lane ] = o;
			}

			if( jok )
			{
				// out[j] = FIR7 over G[ clamp( j - e +- i ) ]
				const int glast = A.g_len - 1;
				const int c = j - A.e;
				o = A.f[ 0 ] * mbuf[ gp_clamp( c, glast ) - mlo ];
				o = o + A.f[ 1 ] * ( mbuf[ gp_clamp( c + 1, glast ) - mlo ] +
					mbuf[ gp_clamp( c - 1, glast ) - mlo ]);
				o = o + A.f[ 2 ] * ( mbuf[ gp_clamp( c + 2, glast ) - mlo ] +
					mbuf[ gp_clamp( c - 2, glast ) - mlo ]);
				o = o + A.f[ 3 ] * ( mbuf[ gp_clamp( c + 3, glast ) - mlo ] +
					mbuf[ gp_clamp( c - 3, glast ) - mlo ]);
			}
		}

		if( LANC && P.lout.on != 0 )
		{
			gp_store_lancir_row< OUTK >( P.lout, r - P.dst_row0, j, o, jok );
		}
		else
		if( jok )
		{
#ifdef GP_DBG
			if( !( P.dbg & 1 ) || o.x == 1234.5f )
#endif
			*(f4*) ( P.dst + (long) ( r - P.dst_row0 ) * P.dst_ss +
				(long) j * 4 ) = o;
		}

		if( SRC != 0 && r + 1 < r1 )
		{
			// row r + 1 (loaded a row ago) into its buffer, row r + 2 out
			t_store(( buf + 1 ) & ( GH_NB - 1 ));

			if( r + 2 < r1 )
			{
				t_load( r + 2 );
			}
		}
	}
}

// ---------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------

// Whether a pass takes the accumulation kernel where the axis has one. Axes
// that downsize by 1 < k < 2 (13 .. 25 taps over the zero-stuffed view) have had
// one since round 4; measured against the gather kernels on one box
// (3840x2160 sources): RGB uint8 k = 1.5 0.109 vs 0.151 ms, k = 1.92 0.099 vs
// 0.141; float RGBA on the EXACT kernels k = 1.5 0.118 vs 0.122, k = 1.75 0.109
// vs 0.113, k = 1.92 0.111 vs 0.116 -- `always`: integer and float RGBA
// sources. Float pixels of 1-3 channels run optimistically (gpass_route: two
// more launches) and take it from k = 1.7 on (RGBA, optimistic: k = 1.5 0.139
// vs 0.126, k = 1.75 0.113 vs 0.115, k = 1.92 0.111 vs 0.118).
// Round 6: FLOAT RGBA sources on 1 < k < 2 axes go back to the gather kernels
// (`frgba`). k_gh's gather-then-FIR form ran its 13 .. 25 taps through the
// any-count variant -- a wave-uniform branch and an LDS round trip per block of
// four taps; with the tap count a compile-time constant (the whole window read at
// once, as the LANCIR variants have had it since round 5) the horizontal pass of
// 3840x2160 -> 2560x1440 takes 51 instead of 70 us and the plan 0.097 instead of
// 0.118 ms on the accumulation kernels (same box; -> 2000x1125 0.092 vs 0.111,
// -> 2200x1238 0.091 vs 0.107: profiles/r06_gh_post/). Integer sources keep the
// branch-free accumulation kernels, which read them raw (RGB uint8 k = 1.5:
// 0.104 vs 0.133). AVIRHIP_SA_ZS_FRGBA=1: the round-5 routing (A/B).
static bool sa_wanted( const SAData* sa, const bool always,
	const bool frgba )
{
	static const double kmin = ( getenv( "AVIRHIP_SA_ZS_KMIN" ) != nullptr ?
		atof( getenv( "AVIRHIP_SA_ZS_KMIN" )) : 1.7 ); // (tuning aid)
	static const bool zs_frgba = ( getenv( "AVIRHIP_SA_ZS_FRGBA" ) != nullptr &&
		atoi( getenv( "AVIRHIP_SA_ZS_FRGBA" )) != 0 );

	if( sa != nullptr && frgba && !zs_frgba && sacc_is_zs( sa ))
	{
		return( false );
	}

	return( sa != nullptr && ( always || !sacc_is_zs( sa ) ||
		sacc_k( sa ) >= kmin ));
}

struct GPData
{
	GPAxisHost h, v;     // AVIR: H pass first; LANCIR: V pass first
	SAData* sa_h;        // downsizing axes: by-sample tables (sacc.hip), or
	SAData* sa_v;        // nullptr where the gather kernels run the axis
	bool h_geom, v_geom; // the gather kernels' launch geometry exists
	int* d_hseg;
	int h_nstrips, h_ow, h_nseg, h_sbuf, h_mbuf;
	// k_gh2 (gpass_h2.hip: two gather outputs per lane on 1 < k < 2 axes):
	// its own strips of up to 122 outputs; h2_ow == 0: no such geometry
	int* d_h2seg;
	int h2_nstrips, h2_ow, h2_nseg, h2_sbuf, h2_mbuf;
	int v_blk, v_rs, v_rc;
	float* mid;          // intermediate image between the passes
	size_t mid_bytes;
	unsigned int* nf_flag; // float sources on the branch-free kernels: the alarm
	// LANCIR upsizing in one launch (lfuse.hip): strips whose source segment is
	// at most 64 pixels
	int lf_ow, lf_nstrips;
	int* d_lfseg;
	float* d_lfvtab;     // [v.g_len][8]: vertical coefficient rows per output
	std::vector< void* > allocs;
};

static int next_pow2( int v )
{
	int p = 2;
	while( p < v ) p <<= 1;
	return( p );
}

// Whether the gather kernels can run an axis of a call, from the plan's data
// alone. Horizontal: the strips exist; a raw source is read in at most four
// pieces a row, by the AVIR variants only. Vertical: the rings fit; an output
// stage handles whole pixels, whose rings are twice as long.
static bool h_gather_takes( const GPData* D, const bool has_raw )
{
	return( D -> h_geom && ( !has_raw || ( D -> h_nseg <= 4 && !D -> h.a.lanc )));
}

static bool v_gather_takes( const GPData* D, const bool has_out )
{
	return( D -> v_geom && ( !has_out || gv_whole_px_fits( D -> v_rs, D -> v_rc )));
}

// Recognises PRE / POST / NONE in a lowered AVIR axis.
static bool match_avir_axis( const LAxis& ax, GPAxisHost& H )
{
	H.ok = false;
	const LOp* fir = nullptr;
	const LOp* gat = nullptr;
	int mode;

	if( ax.ops.size() == 2 && ax.ops[ 0 ].type == OP_FIR &&
		ax.ops[ 1 ].type == OP_GATHER )
	{
		mode = GP_PRE; fir = &ax.ops[ 0 ]; gat = &ax.ops[ 1 ];
	}
	else
	if( ax.ops.size() == 2 && ax.ops[ 0 ].type == OP_GATHER &&
		ax.ops[ 1 ].type == OP_FIR )
	{
		mode = GP_POST; gat = &ax.ops[ 0 ]; fir = &ax.ops[ 1 ];
	}
	else
	if( ax.ops.size() == 1 && ax.ops[ 0 ].type == OP_GATHER )
	{
		mode = GP_NONE; gat = &ax.ops[ 0 ];
	}
	else
	{
		return( false );
	}

	if( fir != nullptr && ( fir -> rf != 1 || fir -> lat != 3 ||
		fir -> view != VIEW_CLAMP || fir -> e < 0 || fir -> e > 3 ))
	{
		return( false );
	}

	if( gat -> view == VIEW_RAW || gat -> maxtaps < 2 || gat -> maxtaps > 64 )
	{
		return( false );
	}

	for( int j = 0; j < gat -> out_len; j++ )
	{
		if( gat -> h_ntaps[ j ] != gat -> maxtaps )
		{
			return( false ); // (a shorter row would multiply padded taps)
		}

		if( j > 0 && gat -> h_start[ j ] < gat -> h_start[ j - 1 ])
		{
			return( false );
		}
	}

	GPAxis& A = H.a;
	memset( &A, 0, sizeof( A ));
	A.mode = mode; A.lanc = 0; A.nt = gat -> maxtaps;
	A.in_len = ax.src_len;
	A.view_mmax = ( gat -> view == VIEW_ZS ? gat -> zs_mmax : 0x7fffffff );
	A.g_len = gat -> out_len;
	A.out_len = ax.dst_len;
	A.e = ( fir != nullptr ? fir -> e : 0 );
	A.c_len = 0;

	if( mode == GP_PRE )
	{
		// (the window algebra below is written for e == lat == 3: C[m] reads
		// S[clamp(m) - 6 .. clamp(m)])
		if( fir -> e != 3 || fir -> in_len != ax.src_len ||
			gat -> in_len != fir -> out_len ||
			fir -> out_len != ax.src_len + 2 * fir -> e )
		{
			return( false );
		}

		A.c_len = fir -> out_len;
	}
	else
	{
		if( gat -> in_len != ax.src_len )
		{
			return( false );
		}

		if( mode == GP_POST && ( fir -> in_len != gat -> out_len ||
			fir -> out_len != ax.dst_len ))
		{
			return( false );
		}
	}

	if( fir != nullptr )
	{
		for( int i = 0; i < 4; i++ )
		{
			A.f[ i ] = fir -> h_flt[ i ];
		}
	}

	A.start = gat -> d_start;
	A.coef = gat -> d_coef;
	A.fidx = nullptr;
	H.start = gat -> h_start;
	H.h_coef = gat -> h_coef.data();
	H.h_fidx = nullptr;
	H.ok = true;
	return( true );
}

static void match_lancir_axis( const LancirAxisDev& L, int order,
	GPAxisHost& H )
{
	GPAxis& A = H.a;
	memset( &A, 0, sizeof( A ));
	H.ok = ( L.kernel_len >= 2 && L.kernel_len <= 64 &&
		( L.kernel_len & 1 ) == 0 );

	A.mode = GP_NONE; A.lanc = ( order >= 1 && order <= 3 ? order : 4 );
	A.nt = L.kernel_len;
	A.in_len = L.src_len; A.view_mmax = 0x7fffffff;
	A.g_len = L.dst_len; A.out_len = L.dst_len; A.e = 0;
	A.start = L.d_start; A.coef = L.d_flt; A.fidx = L.d_fidx;
	H.start = L.h_start;
	H.h_coef = L.h_flt.data();
	H.h_fidx = L.h_fidx.data();

	for( size_t j = 1; j < H.start.size(); j++ )
	{
		H.ok &= ( H.start[ j ] >= H.start[ j - 1 ]);
	}
}

bool fused_dn_both( const avirhip_plan* p ); // fused.hip

int gpass_prepare( avirhip_plan* p )
{
	p -> gpass = nullptr;

	if( p -> ch != 4 || getenv( "AVIRHIP_NO_GPASS" ) != nullptr )
	{
		return( AVIRHIP_OK );
	}

	GPData* D = new GPData();
	D -> mid = nullptr; D -> mid_bytes = 0; D -> d_hseg = nullptr;
	D -> d_h2seg = nullptr; D -> h2_ow = 0; D -> h2_nstrips = 0;
	D -> h2_nseg = 0; D -> h2_sbuf = 0; D -> h2_mbuf = 0;
	D -> nf_flag = nullptr;
	D -> lf_ow = 0; D -> lf_nstrips = 0; D -> d_lfseg = nullptr;
	D -> d_lfvtab = nullptr;
	D -> sa_h = nullptr; D -> sa_v = nullptr;
	D -> h_geom = false; D -> v_geom = false;

	if( p -> is_lancir )
	{
		// (l_order: the channel count whose summation order applies -- the
		// padded RGBA inner plan of a 1-3 channel image keeps the image's)
		match_lancir_axis( p -> lv, p -> l_order, D -> v );
		match_lancir_axis( p -> lh, p -> l_order, D -> h );

		if( p -> l_order != 4 && ( p -> lv.kernel_len < 4 ||
			p -> lh.kernel_len < 4 ))
		{
			D -> h.ok = false;
		}

		// the float pipeline only: integer I/O and the OutMul / clamp output
		// stage stay with the generic kernels
		if( p -> in_type != AVIRHIP_F32 || p -> out_type != AVIRHIP_F32 ||
			!p -> l_unity )
		{
			D -> h.ok = false;
		}
	}
	else
	{
		match_avir_axis( p -> h, D -> h );
		match_avir_axis( p -> v, D -> v );
	}

	if( !D -> h.ok || !D -> v.ok )
	{
		delete D;
		return( AVIRHIP_OK );
	}

	{
		int rc = sacc_prepare_axis( D -> h, D -> allocs, &D -> sa_h );
		if( rc == 0 ) rc = sacc_prepare_axis( D -> v, D -> allocs, &D -> sa_v );

		if( rc != 0 )
		{
			p -> gpass = D;
			gpass_release( p );
			return( rc );
		}
	}

	// ---- horizontal pass geometry: strips of `ow` outputs whose gather
	// inputs (and, PRE, their FIR inputs) fit 64-lane pieces
	{
		const GPAxis& A = D -> h.a;
		const std::vector< int >& st = D -> h.start;
		// Strip width: every candidate that fits is priced by the pixels a
		// wave moves and the lanes it keeps busy per output -- LDS-DMA pieces
		// are 64 pixels whatever the segment needs (a 67-pixel segment costs
		// two; the H pass of 1920 -> 2500 moved 88 MB for a 33 MB source with
		// 64-output strips), and a strip narrower than the wave idles lanes.
		int ow = 0;
		std::vector< int > seg;
		int nstrips = 0, maxs = 0, maxm = 0;
		double best_cost = 0.0;

		for( int cw = ( A.mode == GP_POST ? 58 : 64 ); cw >= 8; cw-- )
		{
			const int cn = ( A.out_len + cw - 1 ) / cw;
			std::vector< int > cseg( (size_t) cn * 4, 0 );
			int cs = 0, cm = 0;

			for( int s = 0; s < cn; s++ )
			{
				const int ja = s * cw;
				const int jb = std::min( A.out_len, ja + cw ) - 1;
				int ga = ja, gb = jb;

				if( A.mode == GP_POST )
				{
					ga = std::max( 0, std::min( ja - A.e - 3, A.g_len - 1 ));
					gb = std::max( 0, std::min( jb - A.e + 3, A.g_len - 1 ));
				}

				// gather input range
				int ia = st[ ga ], ib = st[ gb ] + A.nt - 1;
				int sa = ia, sb = ib, ma = ga, mb = gb;

				if( A.mode == GP_PRE )
				{
					// C[m] reads S[clamp(m) - 6 .. clamp(m)]
					ma = ia; mb = ib;
					sa = std::max( 0, std::min( ia, A.c_len - 1 )) - 2 * A.e;
					sb = std::max( 0, std::min( ib, A.c_len - 1 ));
				}

				cseg[ s * 4 ] = sa; cseg[ s * 4 + 1 ] = sb - sa + 1;
				cseg[ s * 4 + 2 ] = ma; cseg[ s * 4 + 3 ] = mb - ma + 1;
				cs = std::max( cs, sb - sa + 1 );
				cm = std::max( cm, mb - ma + 1 );
			}

			// the FIR and POST stages run one buffer entry per lane and pass
			if( cs > 256 || ( A.mode != GP_NONE && cm > 64 ))
			{
				continue;
			}

			const double cost = ((( cs + 63 ) / 64 ) * 64 + 64 ) / (double) cw;

			if( ow == 0 || cost < best_cost )
			{
				best_cost = cost;
				ow = cw; nstrips = cn; maxs = cs; maxm = cm;
				seg.swap( cseg );
			}
		}

		if( ow == 0 && D -> sa_h == nullptr )
		{
			p -> gpass = D;
			gpass_release( p );
			return( AVIRHIP_OK );
		}

		D -> h_geom = ( ow != 0 );
		D -> h_ow = ow;
		D -> h_nstrips = nstrips;
		D -> h_nseg = ( maxs + 63 ) / 64;
		D -> h_sbuf = D -> h_nseg * 64;
		D -> h_mbuf = std::max( 64, (( maxm + 63 ) / 64 ) * 64 );
		void* q = nullptr;
		if( ow != 0 )
		{
		AVIRHIP_HIPCHECK( hipMalloc( &q, seg.size() * sizeof( int )));
		D -> allocs.push_back( q );
		AVIRHIP_HIPCHECK( hipMemcpy( q, seg.data(), seg.size() * sizeof( int ),
			hipMemcpyHostToDevice ));
		D -> d_hseg = (int*) q;
		}
	}

	// ---- ... and the strips of k_gh2: gather-then-FIR axes over the zero-
	// stuffed view (1 < k < 2) with 13 .. 25 taps whose consecutive outputs
	// start 1 or 2 source pixels apart -- a lane evaluates two of them from one
	// window of NT + 2 pixels
	{
		const GPAxis& A = D -> h.a;
		const std::vector< int >& st = D -> h.start;
		bool ok = ( A.mode == GP_POST && !A.lanc && A.nt >= 13 && A.nt <= 25 &&
			A.g_len >= 2 && A.out_len >= 2 );

		for( int g = 0; ok && g + 1 < A.g_len; g++ )
		{
			const int d = st[ g + 1 ] - st[ g ];
			ok = ( d == 1 || d == 2 );
		}

		int ow = 0, nstrips = 0, maxs = 0, maxm = 0;
		std::vector< int > seg;
		double best_cost = 0.0;

		for( int cw = 122; ok && cw >= 16; cw-- )
		{
			const int cn = ( A.out_len + cw - 1 ) / cw;
			std::vector< int > cseg( (size_t) cn * 4, 0 );
			int cs = 0, cm = 0;

			for( int sx = 0; sx < cn; sx++ )
			{
				const int ja = sx * cw;
				const int jb = std::min( A.out_len, ja + cw ) - 1;
				const int ga = std::max( 0, std::min( ja - A.e - 3, A.g_len - 1 ));
				const int gb = std::max( 0, std::min( jb - A.e + 3, A.g_len - 1 ));
				const int sa = st[ ga ], sb = st[ gb ] + A.nt - 1;

				cseg[ sx * 4 ] = sa; cseg[ sx * 4 + 1 ] = sb - sa + 1;
				cseg[ sx * 4 + 2 ] = ga; cseg[ sx * 4 + 3 ] = gb - ga + 1;
				cs = std::max( cs, sb - sa + 1 );
				cm = std::max( cm, gb - ga + 1 );
			}

			if( cs > 256 || cm > 128 )
			{
				continue;
			}

			// (pixels a wave moves by DMA, lanes it keeps busy, per output)
			const double cost = ((( cs + 63 ) / 64 ) * 64 + 64 ) / (double) cw;

			if( ow == 0 || cost < best_cost )
			{
				best_cost = cost;
				ow = cw; nstrips = cn; maxs = cs; maxm = cm;
				seg.swap( cseg );
			}
		}

		if( ow != 0 )
		{
			void* q = nullptr;
			AVIRHIP_HIPCHECK( hipMalloc( &q, seg.size() * sizeof( int )));
			D -> allocs.push_back( q );
			AVIRHIP_HIPCHECK( hipMemcpy( q, seg.data(), seg.size() * sizeof( int ),
				hipMemcpyHostToDevice ));
			D -> d_h2seg = (int*) q;
			D -> h2_ow = ow; D -> h2_nstrips = nstrips;
			D -> h2_nseg = ( maxs + 63 ) / 64;
			D -> h2_sbuf = D -> h2_nseg * 64;
			D -> h2_mbuf = 128;
			(void) maxm;
		}
	}

	// ---- vertical pass geometry: LDS rings hold what the gathers address
	// dynamically, one window plus the row being written
	{
		const GPAxis& A = D -> v.a;
		int rs = 2, rc = 2;

		// tap counts the register-window kernels exist for (launch_gv): no
		// window in LDS at all
		bool rw;

		if( A.lanc )
		{
			rw = ( A.nt >= 6 && A.nt <= 24 && ( A.nt & 1 ) == 0 );
		}
		else
		if( A.mode == GP_PRE )
		{
			rw = ( A.nt == 12 );
		}
		else
		{
			rw = ( A.mode == GP_POST && A.nt >= 13 && A.nt <= 25 );
		}

		if( rw )
		{
			rc = ( A.mode == GP_POST ? 8 : 2 );
		}
		else
		if( A.mode == GP_PRE )
		{
			rc = next_pow2( A.nt + 1 );
		}
		else
		{
			// the window, the row pair being consumed and GV_PF pairs in flight
			rs = next_pow2( A.nt + 2 * GV_PF + 3 );
			rc = ( A.mode == GP_POST ? 8 : 2 );
		}

		// (+ the PRE landing queue: 5 pair slots and one dump slot)
		D -> v_geom = (( rs + rc ) * 512 + GV_QB + 6 * 1024 <= 64 * 1024 );

		if( !D -> v_geom && D -> sa_v == nullptr )
		{
			p -> gpass = D;
			gpass_release( p );
			return( AVIRHIP_OK );
		}

		D -> v_blk = 1; D -> v_rs = rs; D -> v_rc = rc;
	}

	// ---- LANCIR upsizing, both kernels 6 taps: the fused launch's strips --
	// the widest whose source segments fit one 64-pixel piece
	if( p -> is_lancir && D -> h.a.lanc != 0 && D -> v.a.lanc == D -> h.a.lanc &&
		D -> h.a.nt == 6 && D -> v.a.nt == 6 &&
		getenv( "AVIRHIP_NO_LFUSE" ) == nullptr )
	{
		const GPAxis& A = D -> h.a;
		const std::vector< int >& st = D -> h.start;

		for( int cw = 64; cw >= 16 && D -> lf_ow == 0; cw-- )
		{
			const int cn = ( A.out_len + cw - 1 ) / cw;
			std::vector< int > seg( (size_t) cn * 2, 0 );
			bool fits = true;

			for( int s = 0; s < cn && fits; s++ )
			{
				const int ja = s * cw;
				const int jb = std::min( A.out_len, ja + cw ) - 1;
				const int sa = st[ ja ], sb = st[ jb ] + A.nt - 1;
				seg[ s * 2 ] = sa; seg[ s * 2 + 1 ] = sb - sa + 1;
				fits = ( sb - sa + 1 <= 64 );
			}

			if( fits )
			{
				void* q = nullptr;
				AVIRHIP_HIPCHECK( hipMalloc( &q, seg.size() * sizeof( int )));
				D -> allocs.push_back( q );
				AVIRHIP_HIPCHECK( hipMemcpy( q, seg.data(), seg.size() *
					sizeof( int ), hipMemcpyHostToDevice ));
				D -> d_lfseg = (int*) q;

				// the vertical axis' coefficient rows, one per OUTPUT row
				const GPAxis& V = D -> v.a;
				std::vector< float > vt( (size_t) V.g_len * 8, 0.0f );

				for( int g = 0; g < V.g_len; g++ )
				{
					memcpy( &vt[ (size_t) g * 8 ], D -> v.h_coef +
						(size_t) D -> v.h_fidx[ g ] * V.nt, V.nt * sizeof( float ));
				}

				AVIRHIP_HIPCHECK( hipMalloc( &q, vt.size() * sizeof( float )));
				D -> allocs.push_back( q );
				AVIRHIP_HIPCHECK( hipMemcpy( q, vt.data(), vt.size() *
					sizeof( float ), hipMemcpyHostToDevice ));
				D -> d_lfvtab = (float*) q;
				D -> lf_ow = cw; D -> lf_nstrips = cn;
			}
		}
	}

	// row offsets travel as 32-bit byte offsets
	const long mid_w = ( p -> is_lancir ? p -> src_w : p -> new_w );
	const long mid_h = ( p -> is_lancir ? p -> new_h : p -> src_h );

	if( (long) p -> src_h * p -> src_stride * 4 >= ( 1L << 31 ) ||
		(long) p -> src_h * p -> src_w * 16 >= ( 1L << 31 ) ||
		mid_h * mid_w * 16 >= ( 1L << 31 ))
	{
		p -> gpass = D;
		gpass_release( p );
		return( AVIRHIP_OK );
	}

	D -> mid_bytes = (size_t) mid_w * mid_h * 16;
	p -> gpass = D;
	return( AVIRHIP_OK );
}

void gpass_release( avirhip_plan* p )
{
	GPData* D = (GPData*) p -> gpass;

	if( D != nullptr )
	{
		for( size_t i = 0; i < D -> allocs.size(); i++ )
		{
			(void) hipFree( D -> allocs[ i ]);
		}

		sacc_release_axis( D -> sa_h );
		sacc_release_axis( D -> sa_v );
		delete D;
	}

	p -> gpass = nullptr;
}

bool gpass_ok( const avirhip_plan* p )
{
	return( p -> gpass != nullptr );
}

// Whether the pass kernels are the fastest path for this plan (measured on
// MI355X, profiles/r02_gpass): LANCIR always; AVIR when both axes upsize (FIR7
// then 12-tap gather) from a float RGBA source -- integer sources keep the
// tiled kernels, whose loader converts them in place of a pack pass, and the
// long-tap downsizing chains are still faster there too.
static bool sa16_wanted( const avirhip_plan* p, const GPData* D );
static long sa16_auto_minpix();

bool gpass_preferred( const avirhip_plan* p )
{
	const GPData* D = (const GPData*) p -> gpass;

	if( D == nullptr )
	{
		return( false );
	}

	if( p -> is_lancir )
	{
		return( true );
	}

	// both axes downsize by 2 or more: the streaming-accumulation kernel
	// (any source type: its first pass converts)
	// (measured, profiles/r02_sacc: it wins where its first pass replaces the
	// pack pass or a long-tap tile loader -- integer or narrower sources; for
	// float RGBA the gather / whole-ratio kernels stay ahead)
	// (1 < k < 2, round 4: large frames only -- 1920x1080 -> 1280x720 RGB uint8
	// ties with the tiles at 0.061 ms, 1280x720 -> 854x480 loses 0.048 vs 0.037)
	const bool zs_axes = ( sacc_is_zs( D -> sa_h ) || sacc_is_zs( D -> sa_v ));

	if( D -> sa_h != nullptr && D -> sa_v != nullptr && !p -> gamma &&
		( p -> in_type == AVIRHIP_U8 || p -> in_type == AVIRHIP_U16 ||
		( p -> in_type == AVIRHIP_F32 && p -> io_ch != 4 && !zs_axes )) &&
		( !zs_axes || (long) p -> new_w * p -> new_h >= 2000000L ))
	{
		return( true );
	}

	// ... and float sources (any channel count) of large frames: the same
	// kernels run optimistically (gpass_run), 3840x2160 -> 1500x844 RGBA 0.103
	// against 0.125 ms on the tiles, 5184x3456 -> 1920x1280 0.19 against 0.265;
	// at 1920x1080 -> 700x394 the four launches lose (0.065 against 0.045).
	// Whole-number ratios keep their own kernels (dnf.hip: cfg4 0.046 ms).
	if( D -> sa_h != nullptr && D -> sa_v != nullptr && !p -> gamma &&
		p -> in_type == AVIRHIP_F32 && sacc_has_two( D -> sa_h ) &&
		sacc_has_two( D -> sa_v ) && !fused_dn_both( p ) &&
		sa_wanted( D -> sa_h, p -> io_ch == 4, p -> io_ch == 4 ) &&
		sa_wanted( D -> sa_v, p -> io_ch == 4, p -> io_ch == 4 ) &&
		(long) p -> src_w * p -> src_h >= 6000000L )
	{
		return( true );
	}

	// ... and half / bfloat16 sources the accumulation kernels read where they
	// lie (sa16_wanted), both axes theirs: no pack pass, no float copy
	if( D -> sa_h != nullptr && D -> sa_v != nullptr && !zs_axes &&
		sa16_wanted( p, D ) && !fused_dn_both( p ) &&
		(long) p -> src_w * p -> src_h >= sa16_auto_minpix() )
	{
		return( true );
	}

	// both axes upsize: float RGBA sources always; sources that need the pack
	// pass (integer, 1-3 channels, gamma) once the frame is large enough for
	// two more launches not to matter -- 1920x1080 -> 2500x1400 RGB u8: 0.068
	// against 0.094 ms on the tiles (whose loader converts in place), but
	// 640x480 -> 1024x768: 0.036 against 0.032
	// both axes downsize by 1 < k < 2 (zero-stuffed 13 .. 25-tap gathers, then
	// the correction FIR): ahead of the tiles on large frames (3840x2160 ->
	// 2560x1440 RGBA float 0.137 against 0.179 ms), even with them at 1080p
	if( D -> h.a.mode == GP_POST && D -> v.a.mode == GP_POST &&
		(( D -> sa_h == nullptr && D -> sa_v == nullptr ) || zs_axes ))
	{
		return( (long) p -> new_w * p -> new_h >= 2000000L );
	}

	if( D -> h.a.mode != GP_PRE || D -> v.a.mode != GP_PRE )
	{
		return( false );
	}

	if( p -> in_type == AVIRHIP_F32 && p -> io_ch == 4 && !p -> gamma )
	{
		return( true );
	}

	// integer / narrow pixels on both sides without gamma: the two pass
	// kernels read and write the caller's images themselves -- two launches,
	// ahead of the tiles at every size (640x480 -> 1024x768 RGB u8: 0.027
	// against 0.032 ms)
	const bool raw_in = ( !p -> gamma && ( p -> in_type == AVIRHIP_U8 ||
		p -> in_type == AVIRHIP_U16 || p -> in_type == AVIRHIP_F32 ) &&
		D -> h_geom && D -> h_nseg <= 4 );

	const bool fused_out = ( !p -> gamma && (( p -> dither == AVIRHIP_DITHER_DEF &&
		( p -> out_type == AVIRHIP_U8 || p -> out_type == AVIRHIP_U16 )) ||
		p -> out_type == AVIRHIP_F32 ));

	return(( raw_in && fused_out ) ||
		(long) p -> new_w * p -> new_h >= 2000000L );
}

template< int MODE, bool LANC, int SX >
static void launch_gh2( const GHParams& P, int items, size_t lds,
	hipStream_t st )
{
	const int nt = P.ax.nt;
	// (SX: AVIR plans -- the raw source's element type; LANCIR plans -- the
	// output stage's kind, the source is float RGBA)
	constexpr bool FSRC = ( LANC || SX == 0 );

	// (register-resident coefficient rows for the tap counts that occur: 6
	// LANCIR, 12 AVIR upsizing; raw sources only come with AVIR plans)
	if constexpr( FSRC )
	{
		if( nt == 6 )
		{
			hipLaunchKernelGGL(( k_gh< MODE, LANC, 6, SX > ), dim3( items ),
				dim3( 64 ), lds, st, P );
			return;
		}
	}

	if constexpr( FSRC || MODE == GP_PRE )
	{
		if( nt == 12 )
		{
			hipLaunchKernelGGL(( k_gh< MODE, LANC, 12, SX > ), dim3( items ),
				dim3( 64 ), lds, st, P );
			return;
		}
	}

	// (LANCIR downsizing: the even counts up to 24, as gpassv_lanc.hip has them.
	// Through the run-time tap loop a row was 18 dependent LDS round trips: the
	// horizontal pass of CLancIR 5184x3456 -> 1920x1280 took 33 us for 3 us of
	// arithmetic, and ran slower the longer its chunks were)
	if constexpr( LANC && MODE == GP_NONE )
	{
#define GH_L( N ) case N: hipLaunchKernelGGL(( k_gh< MODE, LANC, N, SX > ), \
	dim3( items ), dim3( 64 ), lds, st, P ); return
		switch( nt )
		{
			GH_L( 8 ); GH_L( 10 ); GH_L( 14 ); GH_L( 16 ); GH_L( 18 );
			GH_L( 20 ); GH_L( 22 ); GH_L( 24 );
			default: break;
		}
#undef GH_L
	}

	// (gather-then-FIR7 axes, 1 < k < 2: 13 .. 25 taps. Float RGBA sources get a
	// compile-time tap count -- the whole window read at once, one LDS round
	// trip per row instead of one per block of four taps in the any-count
	// variant below: round 6, NOTEBOOK 10)
	if constexpr( MODE == GP_POST && !LANC && FSRC )
	{
		if( getenv( "AVIRHIP_GH_POST_ANY" ) == nullptr ) // (A/B: the old variant)
		{
#define GH_L( N ) case N: hipLaunchKernelGGL(( k_gh< MODE, LANC, N, SX > ), \
	dim3( items ), dim3( 64 ), lds, st, P ); return
			switch( nt )
			{
				GH_L( 13 ); GH_L( 14 ); GH_L( 15 ); GH_L( 16 ); GH_L( 17 );
				GH_L( 18 ); GH_L( 19 ); GH_L( 20 ); GH_L( 21 ); GH_L( 22 );
				GH_L( 23 ); GH_L( 24 ); GH_L( 25 );
				default: break;
			}
#undef GH_L
		}
	}

	// (... any other count up to 28, and raw sources: one variant with the
	// coefficient row in registers)
	if constexpr( MODE == GP_POST && !LANC )
	{
		if( nt <= 28 )
		{
			hipLaunchKernelGGL(( k_gh< MODE, LANC, -1, SX > ), dim3( items ),
				dim3( 64 ), lds, st, P );
			return;
		}
	}

	hipLaunchKernelGGL(( k_gh< MODE, LANC, 0, SX > ), dim3( items ),
		dim3( 64 ), lds, st, P );
}

// src_kind: 0 float RGBA (LDS-DMA); 1 uint8, 2 uint16, 3 float, 4 half,
// 5 bfloat16 pixels read raw
// (LANCIR plans: 1 / 2 = the output stage stores uint8 RGB / RGBA pixels, 3 =
// half / bfloat16 pixels of 1-4 channels: gp_store_lancir_row's kinds)
template< int MODE, bool LANC >
static void launch_gh( const GHParams& P, int src_kind, int items, size_t lds,
	hipStream_t st )
{
	switch( src_kind )
	{
		case 1: launch_gh2< MODE, LANC, 1 >( P, items, lds, st ); break;
		case 2: launch_gh2< MODE, LANC, 2 >( P, items, lds, st ); break;
		case 3: launch_gh2< MODE, LANC, 3 >( P, items, lds, st ); break;
		case 4: launch_gh2< MODE, LANC, ( LANC ? 0 : 4 ) >( P, items, lds, st );
			break;
		case 5: launch_gh2< MODE, LANC, ( LANC ? 0 : 5 ) >( P, items, lds, st );
			break;
		default: launch_gh2< MODE, LANC, 0 >( P, items, lds, st ); break;
	}
}

// Whether float RGBA rows of this plan's horizontal axis are k_gh2's (run_h;
// the ONE test behind it and behind the routing of half / bfloat16 sources,
// io16_prefers_pack): the geometry exists, from AVIRHIP_GH2_MIN_NT taps (22),
// not AVIRHIP_NO_GH2. (Read per call: the GPU suite runs every form on every
// tap count.)
static bool gh2_wanted( const GPData* D )
{
	const int gh2_min_nt = ( getenv( "AVIRHIP_GH2_MIN_NT" ) != nullptr ?
		atoi( getenv( "AVIRHIP_GH2_MIN_NT" )) : 22 );

	return( D -> h2_ow != 0 && D -> h.a.nt >= gh2_min_nt &&
		getenv( "AVIRHIP_NO_GH2" ) == nullptr );
}

// One horizontal gather pass (k_gh, k_gh2). 1: the pass cannot read `G.raw`.
static int run_h( const GPData* D, const GPPass& G, hipStream_t st )
{
	const ImageRef* const raw = G.raw;
	const int row_lo = G.row_lo, row_hi = G.row_hi;
	GHParams P;
	memset( &P.lout, 0, sizeof( P.lout ));
	P.dbg = 0;
#ifdef GP_DBG
	P.dbg = ( getenv( "AVIRHIP_GP_DBG" ) != nullptr ?
		atoi( getenv( "AVIRHIP_GP_DBG" )) : 0 );
#endif

	if( G.lout != nullptr )
	{
		P.lout = *G.lout;
	}

	P.raw = nullptr; P.raw_ss = 0; P.raw_ch = 0; P.raw_elems = 0;
	int src_kind = 0;

	if( !h_gather_takes( D, raw != nullptr ))
	{
		return( 1 );
	}

	if( raw != nullptr )
	{
		P.raw = raw -> ptr; P.raw_ss = raw -> stride; P.raw_ch = raw -> ch;
		src_kind = ( raw -> type == AVIRHIP_U8 ? 1 :
			( raw -> type == AVIRHIP_U16 ? 2 :
			( raw -> type == AVIRHIP_F16 ? 4 :
			( raw -> type == AVIRHIP_BF16 ? 5 : 3 ))));
		P.raw_elems = (long) ( row_hi - 1 ) * raw -> stride +
			(long) G.src_w * raw -> ch;

		if( P.raw_elems < 4 )
		{
			return( 1 );
		}
	}

	P.src = G.src; P.src_ss = G.src_ss; P.src_w = G.src_w;
	P.dst = G.dst; P.dst_ss = G.dst_ss; P.dst_row0 = G.dst_row0;
	P.dst_w = G.dst_w;
	P.ax = D -> h.a;
	P.row_lo = row_lo; P.row_hi = row_hi;

	// float RGBA rows of a 1 < k < 2 axis with 22 .. 25 taps (k from about 1.7):
	// two outputs per lane (gpass_h2.hip). Same box, three alternations
	// (profiles/r06_gh_post/): 3840x2160 -> 2200x1238 (22 taps) 0.0913 -> 0.0865 ms,
	// -> 2000x1125 (25) 0.0924 -> 0.0861; -> 2560x1440 (19 taps, k = 1.5) LOSES,
	// 0.0976 -> 0.1136: both forms issue the same number of vector instructions
	// per output and run at the same issue rate -- k_gh2 only removes LDS work
	// (reads 2.6 M -> 1.6 M, bank conflicts 7.2 M -> 0.2 M cycles per launch),
	// which binds at k = 1.9 (lanes 30 bytes apart) and not at k = 1.5, where
	// its half as many, twice as long waves cost more than they save.
	// AVIRHIP_NO_GH2 / AVIRHIP_GH2_MIN_NT: A/B (gh2_wanted).
	if( gh2_wanted( D ) && raw == nullptr && G.lout == nullptr )
	{
		P.nstrips = D -> h2_nstrips; P.ow = D -> h2_ow;
		P.seg = D -> d_h2seg; P.nseg = D -> h2_nseg;
		P.sbuf = D -> h2_sbuf; P.mbuf = D -> h2_mbuf;
		const int rows2 = row_hi - row_lo;
		const size_t lds2 = (size_t) ( GH_NB * P.sbuf + P.mbuf ) * 16;
		const int wpc2 = std::max( 1, std::min( 16, (int) ( 160 * 1024 /
			( lds2 + 512 ))));

		P.chunk = balanced_chunk( rows2, P.nstrips, 4, rows2, 2, wpc2, false );

		if( getenv( "AVIRHIP_GH_CHUNK" ) != nullptr ) // tuning aid
		{
			P.chunk = std::max( 1, std::min( atoi( getenv( "AVIRHIP_GH_CHUNK" )),
				rows2 ));
		}

		const int items2 = P.nstrips * (( rows2 + P.chunk - 1 ) / P.chunk );

		if( launch_gh2( P, items2, lds2, st ) == 0 )
		{
			if( getenv( "AVIRHIP_VERBOSE" ) != nullptr )
			{
				fprintf( stderr, "k_gh2: %d items (strips %d, chunk %d)\n",
					items2, P.nstrips, P.chunk );
			}

			AVIRHIP_HIPCHECK( hipGetLastError() );
			return( AVIRHIP_OK );
		}
	}

	P.nstrips = D -> h_nstrips; P.ow = D -> h_ow;
	P.seg = D -> d_hseg; P.nseg = D -> h_nseg;
	P.sbuf = D -> h_sbuf; P.mbuf = D -> h_mbuf;

	const int rows = row_hi - row_lo;
	// (tap counts 6 and 12 keep the coefficient row in registers: no LDS table)
	const bool regcoef = ( P.ax.nt == 6 || P.ax.nt == 12 ||
		( P.ax.lanc && raw == nullptr && P.ax.nt >= 6 && P.ax.nt <= 24 &&
		( P.ax.nt & 1 ) == 0 ) ||
		( P.ax.mode == GP_POST && !P.ax.lanc && P.ax.nt <= 28 ));
	const size_t lds_h = (size_t) ( GH_NB * P.sbuf + P.mbuf ) * 16 +
		( regcoef ? 0 : (size_t) (( P.ax.nt + 3 ) & ~3 ) * 64 * 4 );

	const int wpc = std::max( 1, std::min( 16, (int) ( 160 * 1024 /
		( lds_h + 512 ))));

	// (a chunk's fixed cost: its coefficient row load and three rows of DMA
	// lead, about two rows of work)
	P.chunk = balanced_chunk( rows, P.nstrips, 4, rows, 2, wpc, false );

	if( getenv( "AVIRHIP_GH_CHUNK" ) != nullptr ) // tuning aid
	{
		P.chunk = std::max( 1, std::min( atoi( getenv( "AVIRHIP_GH_CHUNK" )), rows ));
	}

	const int nch = ( rows + P.chunk - 1 ) / P.chunk;
	const int items = P.nstrips * nch;
	const size_t lds = lds_h;

	if( getenv( "AVIRHIP_VERBOSE" ) != nullptr )
	{
		fprintf( stderr, "k_gh: %d items (strips %d, chunk %d)\n", items,
			P.nstrips, P.chunk );
	}
	const GPAxis& A = P.ax;

	if( A.lanc )
	{
		const bool out16 = ( P.lout.on != 0 &&
			dtype_is_float16_kind( P.lout.type ));

		// (the store's kind 0 knows uint8, uint16 and float elements)
		if( P.lout.on != 0 && !out16 && P.lout.type != AVIRHIP_U8 &&
			P.lout.type != AVIRHIP_U16 && P.lout.type != AVIRHIP_F32 )
		{
			return( 1 );
		}

		launch_gh< GP_NONE, true >( P, ( out16 ? 3 : P.lout.on != 0 &&
			P.lout.type == AVIRHIP_U8 && P.lout.ch >= 3 ? P.lout.ch - 2 : 0 ),
			items, lds, st );
	}
	else
	if( A.mode == GP_PRE )
	{
		launch_gh< GP_PRE, false >( P, src_kind, items, lds, st );
	}
	else
	if( A.mode == GP_POST )
	{
		launch_gh< GP_POST, false >( P, src_kind, items, lds, st );
	}
	else
	{
		launch_gh< GP_NONE, false >( P, src_kind, items, lds, st );
	}

	AVIRHIP_HIPCHECK( hipGetLastError() );
	return( AVIRHIP_OK );
}

// Source rows (AVIR: of the H pass' output; LANCIR: unused) the vertical pass
// reads for output rows [row0, row1).
static void v_source_rows( const GPData* D, int row0, int row1, int& a, int& b )
{
	const GPAxis& A = D -> v.a;
	const std::vector< int >& st = D -> v.start;
	int ga = row0, gb = row1 - 1;

	if( A.mode == GP_POST )
	{
		ga = std::max( 0, std::min( row0 - A.e - 3, A.g_len - 1 ));
		gb = std::max( 0, std::min( row1 - 1 - A.e + 3, A.g_len - 1 ));
	}

	a = st[ ga ]; b = st[ gb ] + A.nt - 1;

	if( A.mode == GP_PRE )
	{
		a = std::max( 0, std::min( a, A.c_len - 1 )) - 2 * A.e;
		b = std::max( 0, std::min( b, A.c_len - 1 ));
	}

	a = std::max( 0, std::min( a, A.in_len - 1 ));
	b = std::max( 0, std::min( b, A.in_len - 1 ));
}

// The last source row the first pass of output rows [row0, row1) of an AVIR plan
// reads: run_h's `row_hi - 1`, which bounds a typed source's `raw_elems`.
int gpass_last_src_row( const avirhip_plan* p, int row0, int row1 )
{
	const GPData* D = (const GPData*) p -> gpass;
	int a = 0, b = p -> src_h - 1;

	if( D != nullptr && !p -> is_lancir && row1 > row0 )
	{
		v_source_rows( D, row0, row1, a, b );
	}

	return( b );
}

// LANCIR (an inner plan): whether its vertical pass -- the first one -- reads
// the owner's integer / narrower image as it is (whole-pixel lanes of the
// register-window variants of k_gv: gpass_v_raw_ok, which names the element
// types the loaders know -- uint8, uint16, float, half, bfloat16; k_lf's own
// test, lfuse_takes_raw, asks the same of base and pitch). The owner offers a
// half / bfloat16 image only on this path and not under AVIRHIP_GP_NO_IO16
// (api.cpp, lanc_road).
bool gpass_lancir_takes_raw( const avirhip_plan* p, const ImageRef& img )
{
	const GPData* D = (const GPData*) p -> gpass;
	const int lpath = ( p -> path != 0 ? p -> path : p -> auto_path );
	static const bool off = ( getenv( "AVIRHIP_GV_RAWDMA" ) != nullptr &&
		atoi( getenv( "AVIRHIP_GV_RAWDMA" )) == 0 ); // (A/B: the pack pass instead)

	return( D != nullptr && !off && p -> is_lancir && lpath == 5 &&
		D -> v_geom && D -> h_geom && p -> src_w > 48 &&
		gpass_v_raw_ok( D -> v.a, D -> v_rs, D -> v_rc, img, p -> src_w ));
}

// Whether the first pass reads the caller's image as it is (integer types,
// 1-4 channels): AVIR plans whose horizontal axis streams (sacc.hip).
//
// Half / bfloat16 sources (1-4 channels): k_gh's typed loader knows them
// (gp_load_raw kinds 4, 5) -- the horizontal axis runs the gather kernels with
// a source segment of at most four pieces --, and so do k_sacc / k_sacc2
// (typed loaders 4, 5) where the horizontal axis is theirs with k >= 2 and the
// frame is at or above the floor (sa16_wanted); under the floor the pack pass
// stays in front of them, and a zero-stuffed 1 < k < 2 axis is the gather
// kernels'. Two classes of call whose float RGBA kernels have no typed form
// keep the pack pass as well (io16_prefers_pack).
// AVIRHIP_GP_NO_IO16 (read per call): the pack pass and the output stage for
// every 16-bit image on this path -- A/B timing, differential tests.
bool gpass_io16()
{
	return( getenv( "AVIRHIP_GP_NO_IO16" ) == nullptr );
}

static long gf_minpix()
{
	// (a tuning aid, read by the first call of any plan)
	static const long v = ( getenv( "AVIRHIP_GF_MINPIX" ) != nullptr ?
		atol( getenv( "AVIRHIP_GF_MINPIX" )) : 7000000L );

	return( v );
}

// whether route_avir runs k_gf for a float RGBA source (raw == nullptr)
static bool gf_wanted( const avirhip_plan* p, const GPData* D )
{
	const bool two_pass = (( p -> variant & AVIRHIP_VARIANT_UPG_TWO_PASS ) != 0 );
	// (a forced variant bit 4 = "fused whatever the size": tests)
	const bool fused = (( p -> variant & AVIRHIP_VARIANT_UPG_FUSED ) != 0 );

	return( D -> h.a.mode == GP_PRE &&
		D -> v.a.mode == GP_PRE && D -> h.a.nt == 12 && D -> v.a.nt == 12 &&
		D -> h_geom && !two_pass &&
		((long) p -> new_w * p -> new_h >= gf_minpix() || fused ) &&
		getenv( "AVIRHIP_NO_GFUSE" ) == nullptr );
}

// A half / bfloat16 source where the float RGBA kernel of the call's class has
// no typed form -- k_gf (large upsizing, AVIRHIP_VARIANT_UPG_FUSED) and k_gh2
// (1 < k < 2 from 22 taps) read by LDS-DMA only: pack pass + that kernel, or
// k_gh's typed form ( + k_gv )? The pack pass, both times -- measured in one
// process, the roads alternating over a ring of buffers, RGBA half in and out
// with the narrowing store behind either road (tools/half_timing.py --gpass;
// pack + float RGBA kernel / typed k_gh / both sides unfused, ms):
//   k_gf   1920x1080 -> 5760x3240   0.128 / 0.140 / 0.200
//          3840x2160 -> 6144x3456   0.191 / 0.207 / 0.272
//   k_gh2  3840x2160 -> 2000x1125   0.130 / 0.145 / 0.145
// (bfloat16 the same within 0.003; spread of repeated runs under 0.002.)
// k_gf saves more on `mid` than the pack pass costs; the typed POST form is
// k_gh's any-tap-count variant (190 VGPRs, two waves per SIMD), which loses
// to k_gh2 what the pack pass costs. AVIRHIP_VARIANT_UPG_FUSED always means
// k_gf. AVIRHIP_GP_IO16_GF / AVIRHIP_GP_IO16_GH2 = 1 (read per call): the
// typed road, A/B.
static bool io16_prefers_pack( const avirhip_plan* p, const GPData* D )
{
	if( gf_wanted( p, D ))
	{
		const char* const e = getenv( "AVIRHIP_GP_IO16_GF" );

		return(( p -> variant & AVIRHIP_VARIANT_UPG_FUSED ) != 0 ||
			e == nullptr || atoi( e ) == 0 );
	}

	if( D -> h.a.mode == GP_POST && gh2_wanted( D ))
	{
		const char* const e = getenv( "AVIRHIP_GP_IO16_GH2" );

		return( e == nullptr || atoi( e ) == 0 );
	}

	return( false );
}

// Frames of fewer source pixels keep the pack pass in front of a half /
// bfloat16 source of the accumulation kernels: their float copy is under
// 1 MiB, nothing to gain (AVIRHIP_SA16_MINPIX: a tuning aid, read by the first
// call of any plan).
static long sa16_minpix()
{
	static const long v = ( getenv( "AVIRHIP_SA16_MINPIX" ) != nullptr ?
		atol( getenv( "AVIRHIP_SA16_MINPIX" )) : 65536L );

	return( v );
}

// Whether k_sacc / k_sacc2 read a half / bfloat16 source where it lies (typed
// loaders 4 / 5, row lanes): the horizontal axis is theirs with k >= 2 (not the
// zero-stuffed 1 < k < 2 form, which keeps k_gh / k_gh2), rows of at least one
// group of the exact form, no gamma, the frame at or above the floor. The ONE
// predicate of this road: gpass_takes_raw (and through it api.cpp's `raw`),
// route_avir and gpass_preferred ask it.
static bool sa16_wanted( const avirhip_plan* p, const GPData* D )
{
	return( D != nullptr && !p -> is_lancir && !p -> gamma && gpass_io16() &&
		dtype_is_float16_kind( p -> in_type ) && D -> sa_h != nullptr &&
		!sacc_is_zs( D -> sa_h ) && p -> src_w >= 4 &&
		(long) p -> src_w * p -> src_h >= sa16_minpix() );
}

// Measured in one process, the roads alternating over a ring of buffers, same-
// type half pixels (tools/half_timing.py --sacc, NOTEBOOK 28; bfloat16 within
// 0.003, spread of repeated runs under 0.003; ms):
//                          forced path 5                        automatic
//   RGBA                   typed exact / optimistic / pack road  tiles / path 5
//   5184x3456 -> 1920x1280  0.190 / 0.189 / 0.285                0.351 / 0.187
//   3840x2160 -> 1500x844   0.111 / 0.125 / 0.156                0.169 / 0.110
//   3200x1800 -> 1200x675   0.103 / 0.104 / 0.137                0.129 / 0.102
//   2560x1440 -> 1000x563   0.082 / 0.095 / 0.104                0.093 / 0.082
//   1920x1080 -> 700x394    0.072 / 0.083 / 0.085                0.063 / 0.073
//   640x480 -> 233x175      0.053 / 0.059 / 0.055                0.031 / 0.053
//   320x240 -> 117x88       0.052 / 0.058 / 0.053                --
//   RGB
//   5184x3456 -> 1920x1280  0.206 / 0.179 / 0.287                0.358 / 0.206
//   3840x2160 -> 1500x844   0.117 / 0.115 / 0.155                0.169 / 0.118
//   3200x1800 -> 1200x675   0.106 / 0.097 / 0.136                0.131 / 0.106
//   2560x1440 -> 1000x563   0.082 / 0.086 / 0.101                0.093 / 0.083
//   1920x1080 -> 700x394    0.073 / 0.076 / 0.086                0.065 / 0.073
//   640x480 -> 233x175      0.051 / 0.055 / 0.054                0.031 / 0.051
// The typed exact road is ahead of the pack road at every size down to the
// floor. The automatic path (gpass_preferred) takes such a source, both axes
// on the accumulation kernels, where path 5 is ahead of the tiles: it is at
// 3,686,400 source pixels and is not at 2,073,600.
// AVIRHIP_SA16_AUTO_MINPIX (read when a plan is made): A/B timing.
static long sa16_auto_minpix()
{
	const char* const e = getenv( "AVIRHIP_SA16_AUTO_MINPIX" );

	return( e != nullptr ? atol( e ) : 3600000L );
}

// Whether such a source runs optimistically without being asked to
// (AVIRHIP_VARIANT_SACC_OPTIMISTIC forces it at any size): RGBA never -- the
// exact kernel is as fast or faster at every size, as for float RGBA; pixels
// of 1-3 channels (measured as RGB) from 5,500,000 source pixels on -- ahead
// at 5,760,000, behind at 3,686,400.
static bool sa16_optimistic( const avirhip_plan* p )
{
	return( p -> io_ch < 4 && (long) p -> src_w * p -> src_h >= 5500000L );
}

bool gpass_takes_raw( const avirhip_plan* p )
{
	const GPData* D = (const GPData*) p -> gpass;
	const bool int_src = ( p -> in_type == AVIRHIP_U8 ||
		p -> in_type == AVIRHIP_U16 );

	if( dtype_is_float16_kind( p -> in_type ))
	{
		return( sa16_wanted( p, D ) ||
			( D != nullptr && !p -> is_lancir && !p -> gamma && gpass_io16() &&
			h_gather_takes( D, true ) && !sa_wanted( D -> sa_h, true, true ) &&
			!io16_prefers_pack( p, D )));
	}

	// (the loaders of the accumulation kernels know uint8, uint16 and float
	// elements: double goes through the pack pass)
	return( D != nullptr && !p -> is_lancir &&
		( int_src || p -> in_type == AVIRHIP_F32 ) &&
		( sa_wanted( D -> sa_h, int_src || ( p -> in_type == AVIRHIP_F32 &&
		p -> io_ch == 4 ), p -> in_type == AVIRHIP_F32 && p -> io_ch == 4 ) ||
		h_gather_takes( D, true )));
}

// the owner's output stage (LancirOut) as the kernels' store parameters
static GPLOut gp_make_lout( const avirhip_plan* p, const LancirOut& o )
{
	GPLOut L;
	memset( &L, 0, sizeof( L ));
	L.on = 1; L.type = o.type; L.ch = o.ch; L.unity = o.unity;
	L.out_mul = o.out_mul; L.clampv = o.clampv;
	L.l4 = ( p -> new_w * o.ch ) & ~3;
	L.base = o.dst; L.stride = o.stride;
	return( L );
}

// ---- the route of one call (gpass_route): decided once, as data,
// before anything is launched or allocated (the first row that holds)
//
//   outcome        plan     condition                                       launches
//   refuse         LANCIR   an axis without its gather geometry             --
//   lanc fused     LANCIR   k_lf's strips exist, the fusion pays (lf_pays),   k_lf
//                           k_lf reads `raw` if there is one, not UPG_TWO_PASS
//   lanc two-pass  LANCIR   otherwise (a refused `raw`: 1, as every refusal)  k_gv, k_gh
//   avir fused     AVIR     12-tap upsizing on both axes from float RGBA,   k_gf
//                           7 Mpixels of output or UPG_FUSED, not UPG_TWO_PASS
//   refuse         AVIR     an axis on the gather kernels (sa_wanted says     --
//                           no) without their geometry; a raw source into
//                           k_gh strips of more than 4 pieces; an output
//                           stage on k_gv rings too long for whole-pixel lanes
//   optimistic     AVIR     a float source that is not float RGBA (or       k_sacc2v x2,
//                           SACC_OPTIMISTIC), both axes on the branch-free   k_sacc x2
//                           (half / bfloat16: sa16_optimistic; k_sacc2 first)
//                           accumulation kernels, no SACC_LADDER
//   avir two-pass  AVIR     otherwise: per axis the accumulation kernels    k_sacc* or k_gh /
//                           (exact; integer sources: finite, or ladder)     k_gh2, k_sacc* or
//                           or the gather kernels                           k_gv
//
// An accumulation pass that refuses a call's pointers (sacc_run_axis: 1) falls
// back to the gather kernels of its axis, an optimistic run to the two-pass one.
// Where a LANCIR call's float result goes is not this table's matter: without
// an owner's output stage (`lout`) the last pass writes `dst`, which api.cpp's
// road (lanc_road) made ready before the attempt: `lres`, or the caller's rows.
enum GPOutcome { GPR_REFUSE, GPR_LANC_FUSED, GPR_LANC_TWO_PASS,
	GPR_AVIR_FUSED, GPR_AVIR_OPTIMISTIC, GPR_AVIR_TWO_PASS };
enum GPFamily { GPF_GATHER, GPF_ACC };
enum GPAccForm { GPA_EXACT, GPA_FINITE, GPA_LADDER };

struct GPRoute
{
	GPOutcome outcome;
	GPFamily h, v;   // AVIR two-pass, optimistic: the kernels of each axis ...
	GPAccForm form;  // ... and the form the two-pass accumulation kernels run in
	bool need_mid;   // the intermediate image between two passes
	bool need_alarm; // the plan's alarm word
};

// `raw`, `lout`: gpass_run's; `has_out`: its `iout != nullptr`. No HIP call,
// no allocation.
static const GPRoute gp_refuse = { GPR_REFUSE, GPF_GATHER, GPF_GATHER,
	GPA_EXACT, false, false };

static GPRoute route_lancir( const avirhip_plan* p, const GPData* D,
	const ImageRef* raw, const LancirOut* lout, const double lf_ratio )
{
	GPRoute R = gp_refuse;
	const bool two_pass = (( p -> variant & AVIRHIP_VARIANT_UPG_TWO_PASS ) != 0 );
	const bool fused = (( p -> variant & AVIRHIP_VARIANT_UPG_FUSED ) != 0 );

	// Upsizing from float RGBA pixels: both passes in ONE launch (lfuse.hip)
	// -- LANCIR's vertical-first order makes the fusion free of recomputation
	// (with the owner's image as the source where its rows can travel as
	// bytes). With an INTEGER result the fusion pays up to about 2.7x
	// horizontally (RGBA: 3.2x): the vertical
	// stage works on the 64 / ratio + 6 source columns of a strip's 64 lanes,
	// and the two pass kernels' intermediate image is no longer small against a
	// uint8 result (1920x1080 RGB uint8, same box, fused / two passes: x1.5
	// 0.028 / 0.034 ms, x2.1 0.047 / 0.051, x2.5 0.064 / 0.065, x3 0.092 /
	// 0.086, x4 0.166 / 0.136; RGBA uint8 x3 0.086 / 0.088, x4 0.152 / 0.140;
	// float results: fused wins at every ratio, x3 0.082 / 0.126;
	// profiles/r05_lanc, tools/rounds/r05_lf2.sh; lf_ratio >= 0 replaces both)
	// Half / bfloat16 results (2 bytes per element, gp_store_lancir_row< 3 >):
	// the float rule, fused at every ratio -- 1920x1080 half RGBA in and out,
	// one process, a ring of buffers, k_lf / k_gv + k_gh: x1.5 0.033 / 0.042 ms,
	// x2.5 0.068 / 0.083, x3 0.095 / 0.106, x4 0.162 / 0.164 (tools/
	// half_timing.py --lancgp, NOTEBOOK 27; spread about 0.001, so x4 is a
	// tie). The store has no clamps, roundings or tail rule
	// to run per strip, and the two passes' `mid` costs what it costs a float
	// result; AVIRHIP_LF_INT_RATIO does not move this class.
	const bool lf_pays = ( lout == nullptr || lout -> type == AVIRHIP_F32 ||
		dtype_is_float16_kind( lout -> type ) ||
		(double) p -> new_w <= (double) p -> src_w * ( lf_ratio >= 0.0 ?
		lf_ratio : ( lout -> ch == 4 ? 3.2 : 2.7 )) || fused );
	const bool use_lf = ( D -> lf_ow != 0 && lf_pays && ( raw == nullptr ||
		lfuse_takes_raw( *raw, p -> src_h, p -> src_w )) && !two_pass );

	if( !D -> h_geom || !D -> v_geom )
	{
		return( R );
	}

	R.outcome = ( use_lf ? GPR_LANC_FUSED : GPR_LANC_TWO_PASS );
	R.need_mid = ( R.outcome == GPR_LANC_TWO_PASS );
	return( R );
}

static GPRoute route_avir( const avirhip_plan* p, const GPData* D,
	const ImageRef* raw, const bool has_out )
{
	GPRoute R = gp_refuse;

	// Large upsizing plans of float RGBA sources run both passes in one launch
	// (gfuse.hip): no intermediate image. "Large": a fused chunk repeats the
	// horizontal arithmetic of its 18-row vertical run-in, which the saved
	// FltBuf round trip only pays for once the frame is memory-heavy -- measured
	// (tools/gf_sweep.py, fused / two-pass, profiles/r04_upg/gf_sweep.txt):
	// 1920x1080 x1.3 1.06, x1.6 0.99, x1.9 0.94, x2.3 0.90, x3.0 0.78;
	// 3840x2160 x1.15 0.92, x1.6 0.71; 1280x720 x2.3 1.01, x3.0 0.97 -- the
	// crossing is at about 7 Mpixels of output.
	// AVIRHIP_GF_MINPIX moves it (0: always), AVIRHIP_VARIANT_UPG_TWO_PASS
	// keeps the two pass kernels (tests, A/B timing).
	// (gf_wanted; a half / bfloat16 source of such a call: io16_prefers_pack)
	const bool use_gf = ( raw == nullptr && gf_wanted( p, D ));

	if( use_gf )
	{
		R.outcome = GPR_AVIR_FUSED;
		return( R );
	}

	// an integer image is finite, and so is the FltBuf made from it: both
	// passes may take the branch-free form of the accumulation kernel
	const bool int_src = ( raw != nullptr && ( raw -> type == AVIRHIP_U8 ||
		raw -> type == AVIRHIP_U16 ));
	const bool ladder = (( p -> variant & AVIRHIP_VARIANT_SACC_LADDER ) != 0 );

	// Float sources, both axes streaming: OPTIMISTIC execution. The branch-free
	// kernels are exact for finite samples only; they run first, the last pass
	// raises the plan's alarm word when it emits a NaN or Inf (any non-finite
	// sample inside the call's windows ends up in one: c * Inf and 0 * Inf are
	// never finite; so does an overflow), and the exact kernels follow in the
	// stream behind the alarm -- empty launches for finite images, a complete
	// recomputation of both passes otherwise. (5184x3456 -> 1920x1280 float RGBA:
	// 0.265 ms on the tiles, 0.15 ms this way.)
	// Float RGBA sources (raw == nullptr: they travel by LDS-DMA) do NOT run
	// optimistically unless asked to (AVIRHIP_VARIANT_SACC_OPTIMISTIC): their
	// exact kernels are as fast as the branch-free ones (5184x3456 -> 1920x1280:
	// 127 + 59 us against 131 + 59, profiles/r04_sacc/exact_vs_optimistic.txt)
	// and the two launches behind the alarm cost 9 us a frame. Float pixels of
	// 1-3 channels gain: 0.273 -> 0.198 ms for the same frame as float RGB.
	static const bool no_opt = ( getenv( "AVIRHIP_NO_SACC_OPT" ) != nullptr );
	const bool fsrc0 = ( raw != nullptr ? raw -> type == AVIRHIP_F32 : true );
	static const bool opt_rgba = ( getenv( "AVIRHIP_SACC_OPT_RGBA" ) != nullptr &&
		atoi( getenv( "AVIRHIP_SACC_OPT_RGBA" )) != 0 ); // (tuning aid)
	// A half / bfloat16 source read raw (gpass_takes_raw): a float source that
	// can be non-finite -- never GPA_FINITE, no integer shortcut. Its horizontal
	// axis is k_gh's, or (`sa16`, sa16_wanted) the accumulation kernels': the
	// exact k_sacc< 4 / 5 > alone by default, two launches; optimistically --
	// k_sacc2< 4 / 5 > first -- where AVIRHIP_VARIANT_SACC_OPTIMISTIC asks, as
	// for float RGBA (sa16_optimistic). Its vertical pass reads the float
	// RGBA rows of `mid` and is classified as the pack pass's float RGBA
	// source is.
	const bool h16 = ( raw != nullptr && dtype_is_float16_kind( raw -> type ));
	const bool sa16 = ( h16 && sa16_wanted( p, D ));
	const bool fsrc = ( fsrc0 || sa16 );
	const bool frgba = ( raw == nullptr || h16 );
	const bool opt_wanted = (( raw != nullptr && !h16 ) || opt_rgba ||
		( p -> variant & AVIRHIP_VARIANT_SACC_OPTIMISTIC ) != 0 ||
		( sa16 && sa16_optimistic( p )));

	// (float RGBA -- the exact kernels unless the variant asks)
	const bool sa_always = ( int_src || ( frgba && !opt_wanted ));
	const bool use_sa_h = ( h16 ? sa16 :
		sa_wanted( D -> sa_h, sa_always, raw == nullptr ));
	const bool use_sa_v = sa_wanted( D -> sa_v, sa_always, frgba );

	R.h = ( use_sa_h ? GPF_ACC : GPF_GATHER );
	R.v = ( use_sa_v ? GPF_ACC : GPF_GATHER );
	R.form = ( !int_src ? GPA_EXACT : ladder ? GPA_LADDER : GPA_FINITE );

	// what the plan's data alone refuse, before the first launch
	if(( !use_sa_h && !h_gather_takes( D, raw != nullptr )) ||
		( !use_sa_v && !v_gather_takes( D, has_out )))
	{
		return( R );
	}

	const bool optimistic = ( !int_src && fsrc && !ladder && !no_opt &&
		opt_wanted && use_sa_h && use_sa_v && sacc_has_two( D -> sa_h ) &&
		sacc_has_two( D -> sa_v ));

	R.outcome = ( optimistic ? GPR_AVIR_OPTIMISTIC : GPR_AVIR_TWO_PASS );
	R.need_mid = true;
	R.need_alarm = optimistic;
	return( R );
}

// (the tuning aid is read by the first call of any plan, as gf_minpix's is)
static GPRoute gpass_route( const avirhip_plan* p, const GPData* D,
	const ImageRef* raw, const bool has_out, const LancirOut* lout )
{
	static const double lf_ratio = ( getenv( "AVIRHIP_LF_INT_RATIO" ) != nullptr ?
		atof( getenv( "AVIRHIP_LF_INT_RATIO" )) : -1.0 );

	return( p -> is_lancir ? route_lancir( p, D, raw, lout, lf_ratio ) :
		route_avir( p, D, raw, has_out ));
}

// ---- one function per outcome. What belongs to the call:
struct GPCall
{
	const float* src; long src_stride; // float RGBA rows, unless `raw`
	float* dst;                        // the float result's first band row
	long dst_ss;
	int row0, row1;
	const ImageRef* raw;    // the image the first pass reads instead of `src`
	const GPOut* out;       // AVIR: the last pass stores the caller's pixels
	const LancirOut* lout;  // LANCIR: the last pass runs the owner's output stage
	hipStream_t st;
};

// LANCIR, both passes in one launch (k_lf)
static int run_lanc_fused( const avirhip_plan* p, const GPData* D,
	const GPCall& C )
{
	LFParams G;
	memset( &G, 0, sizeof( G ));
	G.src = C.src; G.src_ss = C.src_stride;
	G.dst = C.dst; G.dst_ss = C.dst_ss; G.dst_row0 = C.row0;
	G.hx = D -> h.a; G.vx = D -> v.a;
	G.row_lo = C.row0; G.row_hi = C.row1;
	G.nstrips = D -> lf_nstrips; G.ow = D -> lf_ow;
	G.seg = D -> d_lfseg; G.vtab = D -> d_lfvtab;

	if( C.raw != nullptr )
	{
		// (an inner plan: the owner's image, read as it is)
		const int esz = (int) dtype_size( C.raw -> type );

		G.raw = C.raw -> ptr; G.raw_ss = C.raw -> stride;
		// (half / bfloat16 pixels: uint16's geometry -- the same bytes per
		// pixel, instruction count and range -- and a conversion of their own)
		G.raw_kind = gp_raw_kind( C.raw -> type );
		G.raw_ch = C.raw -> ch; G.raw_bpp = esz * C.raw -> ch;
		G.raw_bytes = image_dma_bytes( *C.raw, p -> src_h, p -> src_w );
		G.raw_tdn = ( 64 * G.raw_bpp + ( G.raw_bpp & 3 ? 3 : 0 ) + 255 ) >> 8;
	}

	if( C.lout != nullptr )
	{
		G.lout = gp_make_lout( p, *C.lout );
	}

	const int rc = lfuse_launch( G, C.st );

	// (lfuse_launch leaves the chunk it chose in G)
	if( rc == AVIRHIP_OK && getenv( "AVIRHIP_VERBOSE" ) != nullptr )
	{
		fprintf( stderr, "k_lf: %d items (strips %d, chunk %d)\n", G.nstrips *
			(( G.row_hi - G.row_lo + G.chunk - 1 ) / G.chunk ), G.nstrips,
			G.chunk );
	}

	return( rc );
}

// LANCIR, vertical first (lancir.h:601-646): mid = [new_h][src_w], only the
// rows of the band
static int run_lanc_two_pass( const avirhip_plan* p, const GPData* D,
	const GPCall& C )
{
	GPPass V;
	memset( &V, 0, sizeof( V ));
	V.src = C.src; V.src_ss = C.src_stride; V.src_w = p -> src_w;
	V.dst = D -> mid; V.dst_ss = (long) p -> src_w * 4; V.dst_row0 = 0;
	V.dst_w = p -> src_w;
	V.row_lo = C.row0; V.row_hi = C.row1;
	V.raw = C.raw; // (an inner plan: the owner's image, read as it is)

	const int rc = gpass_run_v( D -> v.a, D -> v_blk, D -> v_rs, D -> v_rc, V,
		C.st );

	if( rc != 0 )
	{
		// (1: the kernel refuses the image after all, as any refusal -- the
		// road's next attempt reads the pack pass's float copy; `mid` stays
		// allocated for it)
		return( rc );
	}

	GPPass H;
	memset( &H, 0, sizeof( H ));
	H.src = D -> mid; H.src_ss = V.dst_ss; H.src_w = p -> src_w;
	H.dst = C.dst; H.dst_ss = C.dst_ss; H.dst_row0 = C.row0;
	H.dst_w = p -> new_w;
	H.row_lo = C.row0; H.row_hi = C.row1;
	// (an inner plan: the outer plan's output stage goes into the store of
	// this pass, its result rows are never written)
	GPLOut L;

	if( C.lout != nullptr )
	{
		L = gp_make_lout( p, *C.lout );
		H.lout = &L;
	}

	return( run_h( D, H, C.st ));
}

// AVIR, upsizing on both axes from a float RGBA source: ONE launch runs both
// passes (k_gf), FltBuf never exists
static int run_avir_fused( const avirhip_plan* p, const GPData* D,
	const GPCall& C )
{
	GFParams G;
	memset( &G, 0, sizeof( G ));
	G.src = C.src; G.src_ss = C.src_stride;
	G.dst = C.dst; G.dst_ss = C.dst_ss; G.dst_row0 = C.row0;
	G.hx = D -> h.a; G.vx = D -> v.a;
	G.row_lo = C.row0; G.row_hi = C.row1;
	G.nstrips = D -> h_nstrips; G.ow = D -> h_ow;
	G.seg = D -> d_hseg; G.nseg = D -> h_nseg;
	G.sbuf = D -> h_sbuf; G.mbuf = D -> h_mbuf;

	if( C.out != nullptr )
	{
		G.out = *C.out;
	}

	return( gfuse_launch( G, (double) p -> src_h / p -> new_h, C.st ));
}

// AVIR's passes: horizontal first into mid = FltBuf [src_h][new_w], only the
// source rows [a, b] the band's vertical windows read (v_source_rows).

static int avir_h_acc( const avirhip_plan* p, const GPData* D, const GPCall& C,
	const int a, const int b, const SAForm& F )
{
	SAPass G;
	G.rows = true;
	G.dst = D -> mid; G.d_lane = (long) p -> new_w * 4; G.d_step = 4;
	G.lane_lo = a; G.lane_hi = b + 1; G.out_lo = 0; G.out_hi = p -> new_w;
	G.out = nullptr;

	if( C.raw != nullptr )
	{
		const long es = (long) dtype_size( C.raw -> type );

		G.src = C.raw -> ptr; G.src_type = C.raw -> type;
		G.src_ch = C.raw -> ch; G.live_ch = C.raw -> ch;
		G.s_lane = C.raw -> stride * es; G.s_step = C.raw -> ch * es;
	}
	else
	{
		G.src = C.src; G.src_type = AVIRHIP_F32; G.src_ch = 4;
		G.live_ch = p -> io_ch;
		G.s_lane = C.src_stride * 4; G.s_step = 16;
	}

	return( sacc_run_axis( D -> sa_h, G, F, C.st ));
}

static int avir_v_acc( const avirhip_plan* p, const GPData* D, const GPCall& C,
	const SAForm& F )
{
	SAPass G;
	G.rows = false;
	G.src = D -> mid; G.src_type = AVIRHIP_F32; G.src_ch = 4;
	G.live_ch = p -> io_ch;
	G.s_lane = 16; G.s_step = (long) p -> new_w * 16;
	G.dst = C.dst - (long) C.row0 * C.dst_ss; G.d_lane = 4; G.d_step = C.dst_ss;
	G.lane_lo = 0; G.lane_hi = p -> new_w; G.out_lo = C.row0; G.out_hi = C.row1;
	G.out = C.out;
	return( sacc_run_axis( D -> sa_v, G, F, C.st ));
}

// k_sacc alone, no alarm
static SAForm sa_exact()
{
	SAForm F;
	F.finite = false; F.ladder = false; F.must_two = false;
	F.alarm_set = nullptr; F.alarm_guard = nullptr;
	return( F );
}

static int avir_h( const avirhip_plan* p, const GPData* D, const GPCall& C,
	const GPFamily fam, const int a, const int b, const SAForm& F )
{
	int rc = ( fam == GPF_ACC ? avir_h_acc( p, D, C, a, b, F ) : 1 );

	if( rc == 1 )
	{
		GPPass H;
		memset( &H, 0, sizeof( H ));
		H.src = C.src; H.src_ss = C.src_stride; H.src_w = p -> src_w;
		H.dst = D -> mid; H.dst_ss = (long) p -> new_w * 4; H.dst_row0 = 0;
		H.dst_w = p -> new_w;
		H.row_lo = a; H.row_hi = b + 1;
		H.raw = C.raw;
		rc = run_h( D, H, C.st );
	}

	return( rc );
}

static int avir_v( const avirhip_plan* p, const GPData* D, const GPCall& C,
	const GPFamily fam, const SAForm& F )
{
	int rc = ( fam == GPF_ACC ? avir_v_acc( p, D, C, F ) : 1 );

	if( rc == 1 )
	{
		// (the route has answered this for an axis on the gather kernels: here
		// only behind an accumulation pass that refused the call's pointers)
		if( !v_gather_takes( D, C.out != nullptr ))
		{
			return( 1 );
		}

		GPPass V;
		memset( &V, 0, sizeof( V ));
		V.src = D -> mid; V.src_ss = (long) p -> new_w * 4; V.src_w = p -> new_w;
		V.dst = C.dst; V.dst_ss = C.dst_ss; V.dst_row0 = C.row0;
		V.dst_w = p -> new_w;
		V.row_lo = C.row0; V.row_hi = C.row1;
		V.out = C.out;
		rc = gpass_run_v( D -> v.a, D -> v_blk, D -> v_rs, D -> v_rc, V, C.st );
	}

	return( rc );
}

static int run_avir_two_pass( const avirhip_plan* p, const GPData* D,
	const GPCall& C, const GPRoute& R )
{
	SAForm F = sa_exact();
	F.finite = ( R.form != GPA_EXACT );
	F.ladder = ( R.form == GPA_LADDER );
	int a, b;
	v_source_rows( D, C.row0, C.row1, a, b );

	const int rc = avir_h( p, D, C, R.h, a, b, F );
	return( rc != 0 ? rc : avir_v( p, D, C, R.v, F ));
}

// AVIR, four launches: the branch-free kernels (the first lowers the alarm, the
// second may raise it), then the exact kernels behind the alarm
static int run_avir_optimistic( const avirhip_plan* p, const GPData* D,
	const GPCall& C, const GPRoute& R )
{
	SAForm fast = sa_exact(), exact = sa_exact();
	fast.finite = true; fast.must_two = true; fast.alarm_set = D -> nf_flag;
	exact.alarm_guard = D -> nf_flag;
	int a, b;
	v_source_rows( D, C.row0, C.row1, a, b );

	// (a half / bfloat16 source: its first pass is k_sacc2, whose sources were
	// integers -- it has no code that lowers the alarm; the stream does it)
	if( C.raw != nullptr && dtype_is_float16_kind( C.raw -> type ))
	{
		AVIRHIP_HIPCHECK( hipMemsetAsync( D -> nf_flag, 0, 4, C.st ));
	}

	int rc = avir_h_acc( p, D, C, a, b, fast );
	if( rc == 0 ) rc = avir_v_acc( p, D, C, fast );

	// (AVIRHIP_SACC_OPT_ONLY, read per call: the branch-free launches alone --
	// what they cost, and what they leave where the alarm was due)
	if( rc == 0 && getenv( "AVIRHIP_SACC_OPT_ONLY" ) != nullptr )
	{
		return( rc );
	}

	if( rc == 0 )
	{
		rc = avir_h_acc( p, D, C, a, b, exact );
		return( rc != 0 ? rc : avir_v_acc( p, D, C, exact ));
	}

	// (a pass cannot take the branch-free form: the exact kernels alone)
	return( rc != 1 ? rc : run_avir_two_pass( p, D, C, R ));
}

template< class T >
static int gp_lazy_alloc( avirhip_plan* p, GPData* D, T*& slot,
	const size_t bytes, const bool counted )
{
	if( slot == nullptr )
	{
		void* q = nullptr;
		AVIRHIP_HIPCHECK( hipMalloc( &q, bytes ));
		D -> allocs.push_back( q );
		if( counted ) p -> alloc_bytes += bytes;
		slot = (T*) q;
	}

	return( AVIRHIP_OK );
}

// Runs output rows [row0, row1) of a float RGBA plan. Returns 1 when the call
// cannot take this path (alignment, a pass this plan does not have), so that
// the caller falls back.
// `iout` != nullptr: the caller's integer image (the band's first row) -- the
// last pass converts and stores there (no float result, no epilogue pass);
// returns 1 if this plan's last pass cannot (the caller then runs unfused).
// `raw` != nullptr: the first pass reads that image as it lies instead of
// `src` -- the caller's (AVIR) or the owner's (a LANCIR inner plan).
// `lout` != nullptr (a LANCIR inner plan): the last pass runs the owner's
// output stage and stores into its image; a return of 0 says that it has.
int gpass_run( avirhip_plan* p, const float* src, long src_stride, float* dst,
	int row0, int row1, hipStream_t st, const ImageRef* raw, void* iout,
	const LancirOut* lout )
{
	GPOut O;
	memset( &O, 0, sizeof( O ));

	if( iout != nullptr )
	{
		// (half / bfloat16 pixels of 1-4 channels: narrowed in the store,
		// gp_store_int_row; elements are stored whole, so the image is a
		// multiple of their size -- as gp_store_int stores uint16 elements,
		// through an `unsigned short*`: an even address, up2_run's `io` 2)
		const bool out16 = dtype_is_float16_kind( p -> out_type );

		if( p -> is_lancir || p -> gamma ||
			( p -> out_type != AVIRHIP_F32 &&
			p -> dither != AVIRHIP_DITHER_DEF ) ||
			( p -> out_type != AVIRHIP_U8 && p -> out_type != AVIRHIP_U16 &&
			!( p -> out_type == AVIRHIP_F32 && p -> io_ch < 4 ) && !out16 ) ||
			( p -> out_type == AVIRHIP_U8 && p -> io_ch == 4 &&
			(( (uintptr_t) iout & 3 ) != 0 )) ||
			( p -> out_type == AVIRHIP_U16 && ( (uintptr_t) iout & 1 ) != 0 ) ||
			( out16 && ( !gpass_io16() || ( (uintptr_t) iout & 1 ) != 0 )))
		{
			return( 1 );
		}

		gp_make_out( p, iout, O );

		if( out16 )
		{
			O.fin = 0; // (no integer stage: none of its shortcuts)
		}
	}

	GPData* D = (GPData*) p -> gpass;

	// (`dst` behind an output stage is never written: no alignment asked of it)
	if( D == nullptr || ( iout == nullptr && ( (uintptr_t) dst & 15 )) ||
		( p -> is_lancir && ( p -> new_stride & 3 )) ||
		( raw == nullptr && (( (uintptr_t) src & 15 ) || ( src_stride & 3 ))) ||
		( raw != nullptr && !p -> is_lancir && !gpass_takes_raw( p )) ||
		// (half / bfloat16 elements are loaded whole: run_h refuses fewer
		// than four of them, as it does for every typed source)
		( raw != nullptr && dtype_is_float16_kind( raw -> type ) &&
		( (uintptr_t) raw -> ptr & 1 ) != 0 ))
	{
		return( 1 );
	}

	if( row1 <= row0 )
	{
		return( AVIRHIP_OK );
	}

	const GPRoute R = gpass_route( p, D, raw, iout != nullptr, lout );
	int rc;

	if( R.need_mid && ( rc = gp_lazy_alloc( p, D, D -> mid, D -> mid_bytes,
		true )) != 0 ) return( rc );

	if( R.need_alarm && ( rc = gp_lazy_alloc( p, D, D -> nf_flag, 64,
		false )) != 0 ) return( rc );

	GPCall C;
	C.src = src; C.src_stride = src_stride;
	C.dst = dst;
	C.dst_ss = ( p -> is_lancir ? p -> new_stride : (long) p -> new_w * 4 );
	C.row0 = row0; C.row1 = row1;
	C.raw = raw; C.out = ( iout != nullptr ? &O : nullptr ); C.lout = lout;
	C.st = st;

	switch( R.outcome )
	{
		case GPR_LANC_FUSED: return( run_lanc_fused( p, D, C ));
		case GPR_LANC_TWO_PASS: return( run_lanc_two_pass( p, D, C ));
		case GPR_AVIR_FUSED: return( run_avir_fused( p, D, C ));
		case GPR_AVIR_OPTIMISTIC: return( run_avir_optimistic( p, D, C, R ));
		case GPR_AVIR_TWO_PASS: return( run_avir_two_pass( p, D, C, R ));
		default: return( 1 );
	}
}

} // namespace avirhip
