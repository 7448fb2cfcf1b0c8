// gpassv.hip -- the vertical pass of the general-ratio pass kernels (see
// gpass.hip for the family's description): launch geometry, the AVIR upsizing
// variants of k_gv and the dispatch to the other variant groups.

#include "gpassv_kernel.h"

namespace avirhip {

// Register-window variants exist for the tap counts that occur: 12 for AVIR
// upsizing (FIR7 then gather), 13-25 for AVIR 1 < k < 2 downsizing (gather
// then FIR7, gpassv_post.hip), the even counts 6-24 for LANCIR
// (gpassv_lanc.hip); the LDS-window kernel takes everything else.
static int launch_gv( const GVParams& P, int wp, int items, size_t lds,
	hipStream_t st )
{
	const int nt = P.ax.nt;

	if( P.ax.lanc )
	{
		return( launch_gv_lanc( P, wp, items, lds, st ));
	}
	else
	if( P.ax.mode == GP_PRE )
	{
		if( nt == 12 ) GV_LAUNCH( GP_PRE, false, 12, 16 );
		else GV_LAUNCH( GP_PRE, false, 0, 0 );
	}
	else
	if( P.ax.mode == GP_POST )
	{
		launch_gv_post( P, wp, items, lds, st );
	}
	else
	{
		GV_LAUNCH( GP_NONE, false, 0, 0 );
	}

	return( 0 );
}

bool gpass_v_raw_ok( const GPAxis& A, const int v_rs, const int v_rc,
	const ImageRef& img, const int width )
{
	const long esz = (long) dtype_size( img.type );

	// at least the four elements the loader's bound assumes; dword-aligned base
	// and row pitch, under 2 GiB; a register-window variant of the LANCIR kernels
	// (the LDS-window form keeps a ring of float pixels); whole-pixel lanes
	return( (long) ( A.in_len - 1 ) * img.stride + (long) width * img.ch >= 4 &&
		( (uintptr_t) img.ptr & 3 ) == 0 && (( img.stride * esz ) & 3 ) == 0 &&
		image_dma_bytes( img, A.in_len, width ) != 0 &&
		A.lanc && A.nt >= 6 && A.nt <= 24 && ( A.nt & 1 ) == 0 &&
		gv_whole_px_fits( v_rs, v_rc ) &&
		// ... and an element type raw_px knows (uint8, uint16, float, half,
		// bfloat16)
		gp_raw_kind( img.type ) != 0 );
}

int gpass_run_v( const GPAxis& A_, int v_blk, int v_rs, int v_rc,
	const GPPass& G, hipStream_t st )
{
	const ImageRef* const raw = G.raw;
	const GPOut* const out = G.out;
	const int width = G.src_w;
	GVParams P;
	memset( &P.out, 0, sizeof( P.out ));
	P.raw = nullptr; P.raw_ss = 0; P.raw_ch = 0; P.raw_kind = 1;
	P.raw_elems = 0; P.raw_dma = 0; P.raw_bytes = 0;

	if( raw != nullptr )
	{
		// raw rows travel as bytes by LDS-DMA (k_gv, LVAR bit 1)
		if( !gpass_v_raw_ok( A_, v_rs, v_rc, *raw, width ))
		{
			return( 1 );
		}

		P.raw = raw -> ptr; P.raw_ss = raw -> stride; P.raw_ch = raw -> ch;
		// (half / bfloat16: uint16's element size in `trow_b` and raw_dma)
		P.raw_kind = gp_raw_kind( raw -> type );
		// (rows are `stride` elements apart; the last one ends with its pixels)
		P.raw_elems = (long) ( A_.in_len - 1 ) * raw -> stride +
			(long) width * raw -> ch;
		P.raw_dma = (int) dtype_size( raw -> type ) * raw -> ch;
		P.raw_bytes = image_dma_bytes( *raw, A_.in_len, width );
	}

	if( out != nullptr )
	{
		P.out = *out;
	}

	P.src = G.src; P.src_ss = G.src_ss; P.width = width;
	P.dst = G.dst; P.dst_ss = G.dst_ss; P.dst_row0 = G.dst_row0;
	P.ax = A_;
	P.row_lo = G.row_lo; P.row_hi = G.row_hi;
	P.dbg = ( getenv( "AVIRHIP_GP_DBG" ) != nullptr ? atoi( getenv( "AVIRHIP_GP_DBG" )) : 0 );
	P.blk = v_blk; P.rs = v_rs; P.rc = v_rc;

	// whole-pixel lanes (64-pixel strips) wherever the image is wide enough
	// to fill them and the rings stay within 64 KiB
	int wp = ( width > 48 && gv_whole_px_fits( P.rs, P.rc ) ? 2 : 1 );

	if( getenv( "AVIRHIP_GV_WP" ) != nullptr ) // tuning aid
	{
		wp = ( atoi( getenv( "AVIRHIP_GV_WP" )) == 2 &&
			gv_whole_px_fits( P.rs, P.rc ) ? 2 : 1 );
	}

	if( out != nullptr || raw != nullptr )
	{
		// the integer output stage and the raw-source loader handle whole
		// pixels
		if( !gv_whole_px_fits( P.rs, P.rc ))
		{
			return( 1 );
		}

		wp = 2;
	}

	if( wp == 1 )
	{
		// half-pixel lanes (images narrower than 49 pixels, or windows too
		// long for whole-pixel rings) only exist as the LDS-window kernel:
		// its rings hold the window, whatever the plan sized them for
		int rs = 2, rc = 2;

		if( P.ax.mode == GP_PRE )
		{
			rc = 2;
			while( rc < P.ax.nt + 1 ) rc <<= 1;
		}
		else
		{
			while( rs < P.ax.nt + 2 * GV_PF + 3 ) rs <<= 1;
			rc = ( P.ax.mode == GP_POST ? 8 : 2 );
		}

		if(( rs + rc ) * 512 + GV_QB + 6 * 1024 > 64 * 1024 )
		{
			return( 1 );
		}

		P.rs = rs; P.rc = rc;
	}

	const int rowb = wp * 512;
	P.nstrips = ( width + 32 * wp - 1 ) / ( 32 * wp );

	// chunk height: a chunk's first window (NT rows, + 6 of FIR warm-up) is
	// fed before its first output; its coefficient rows and positions live
	// in LDS (<= 6 KiB)
	const int rows = G.row_hi - G.row_lo;
	const int ntp = ( P.ax.nt + 3 ) & ~3;
	const int gextra = ( P.ax.mode == GP_POST ? 7 : 0 );
	const int maxg = std::max( gextra + 1, 6144 / ( ntp * 4 + 4 ));
	// warm-up in units of output rows (a fed row costs about a third of one)
	const int warm_div = ( getenv( "AVIRHIP_GV_WARMDIV" ) != nullptr ?
		std::max( 1, atoi( getenv( "AVIRHIP_GV_WARMDIV" ))) : 3 );

	const int warm = std::max( 1, (int) ( (long) ( P.ax.nt + 6 ) *
		std::max( 1, P.ax.out_len ) / std::max( 1, P.ax.in_len ) / warm_div ));

	const size_t lds_guess = (size_t) ( P.rs + P.rc ) * rowb + GV_QB + 3072;
	const int wpc = std::max( 1, std::min( 16, (int) ( 160 * 1024 /
		( lds_guess + 512 ))));

	// (chunks down to 4 rows: a small frame -- 640x480 -> 1024x768 -- runs
	// faster as two short waves per SIMD than as one of 12 rows, 0.0231 ->
	// 0.0193 ms; tools/gp_solo_sweep.sh)
	P.chunk = balanced_chunk( rows, P.nstrips, 4, maxg - gextra, warm, wpc,
		true );

	if( getenv( "AVIRHIP_GV_CHUNK" ) != nullptr ) // tuning aid
	{
		P.chunk = std::max( 1, std::min( atoi( getenv( "AVIRHIP_GV_CHUNK" )),
			maxg - gextra ));
	}

	const int nch = ( rows + P.chunk - 1 ) / P.chunk;
	const int items = P.nstrips * nch;

	if( getenv( "AVIRHIP_VERBOSE" ) != nullptr )
	{
		fprintf( stderr, "k_gv: %d items (strips %d, chunk %d, clamp %d, nt %d, "
			"post %d)\n", items, P.nstrips, P.chunk, maxg - gextra, P.ax.nt,
			( gextra != 0 ? 1 : 0 ));
	}
	const size_t lds = (size_t) ( P.rs + P.rc ) * rowb + GV_QB +
		(size_t) ( P.chunk + gextra ) * ( ntp * 4 + 4 ) + 64;

#ifdef GP_DBG
	{
		static int once = 0;
		if( !once++ ) fprintf( stderr, "k_gv: wp %d strips %d chunk %d items %d "
			"lds %zu nt %d mode %d\n", wp, P.nstrips, P.chunk, items, lds,
			P.ax.nt, P.ax.mode );
	}
#endif
	// (1: no kernel of the variant group takes this plan -- the caller falls
	// back: api.cpp's road goes on to its next attempt, behind the pack pass)
	if( launch_gv( P, wp, items, lds, st ) != 0 )
	{
		return( 1 );
	}

	AVIRHIP_HIPCHECK( hipGetLastError() );
	return( AVIRHIP_OK );
}

} // namespace avirhip
