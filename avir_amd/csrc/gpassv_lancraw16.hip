// gpassv_lancraw16.hip -- the raw-source variants for half / bfloat16 pixels
// (inner plans of CLancIR images with 16-bit float elements; whole-pixel
// lanes). The rows travel as bytes exactly as uint16 rows do -- the same bytes
// per pixel, DMA, landing queue and waits -- and a lane widens its pixel when
// it reads the queue (raw_px, LVAR bit 3). A translation unit of its own: the
// uint16 / float variants of gpassv_lancraw.hip are not recompiled with
// another case in their step.
#include "gpassv_kernel.h"

namespace avirhip {

// returns 1 when no variant exists for the plan's tap count (nothing launched)
int launch_gv_lanc_raw16( const GVParams& P, int items, size_t lds,
	hipStream_t st )
{
	const int nt = P.ax.nt;

	if( P.raw_kind != 4 && P.raw_kind != 5 )
	{
		return( 1 );
	}

	switch( nt )
	{
		case 6: GV_LAUNCH_LR16( 6, 8 ); break;
		case 8: GV_LAUNCH_LR16( 8, 8 ); break;
		case 10: GV_LAUNCH_LR16( 10, 16 ); break;
		case 12: GV_LAUNCH_LR16( 12, 16 ); break;
		case 14: GV_LAUNCH_LR16( 14, 16 ); break;
		case 16: GV_LAUNCH_LR16( 16, 16 ); break;
		case 18: GV_LAUNCH_LR16( 18, 32 ); break;
		case 20: GV_LAUNCH_LR16( 20, 32 ); break;
		case 22: GV_LAUNCH_LR16( 22, 32 ); break;
		case 24: GV_LAUNCH_LR16( 24, 32 ); break;
		// (other tap counts: gpass_v_raw_ok refuses them, as for every raw kind)
		default: return( 1 );
	}

	return( 0 );
}

} // namespace avirhip
