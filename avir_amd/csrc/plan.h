// plan.h -- internal (not part of the C ABI): the lowered, device-resident form
// of a plan and the launch entry points of the kernel families.
//
// Lowering turns the reference-shaped step list of include/avirhip.h into a
// chain of "ops" per axis. Every op produces a materialised array of pixels
// along the axis; it reads its input through a *view* that reproduces, by
// index algebra, what the reference obtains by writing replicated/zeroed
// prefix and suffix pixels into its flip-flop buffers:
//
//   VIEW_CLAMP  in[clamp(i, 0, in_len-1)]          (prepareInBuf, avir.h:3227)
//   VIEW_ZS     zero-stuffed 2x view of a clamped input; the consumer reads
//               only the even (non-zero) slots 2m -> in[clamp(m)], and slots
//               past the last replicated pixel read 0 (doUpsample no-filter
//               branch, avir.h:3260-3402)
//   VIEW_RAW    in[i + prefix] of a materialised filtered-upsample buffer
//
#pragma once
#include "waits.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <atomic>
#include <mutex>
#include <thread>
#include "../../include/avirhip.h"

// The (int) cast of the reference's x86-64 build (cvttss2si), which avir::round
// (avir.h:130-135) is made of: a value the 32-bit integer cannot hold -- NaN
// included -- converts to INT_MIN, the "integer indefinite" (C++ leaves it
// undefined; the parity target is that build). gfx950's v_cvt_i32_f32
// saturates instead, so float images with HDR-sized or non-finite samples would
// give other integer pixels: +1e10 -> 0 and -1e10 -> the maximum in the
// reference (round() returns -2^31 / +2^31, then the clamp).
__host__ __device__ __forceinline__ int avirhip_x86_cvtt( const float f )
{
	return( fabsf( f ) < 2147483648.0f ? (int) f : ( -2147483647 - 1 ));
}

// ... for the output stages that drop avir::round's negative branch (whatever it
// returns for -2^31 < d < 0 the clamp turns into 0): `t` is the clamped result
// computed with the saturating cast from round()'s argument `a`; beyond the
// int range the reference's round() is -2^31 for positive and +2^31 for
// negative arguments, i.e. 0 and the maximum after the clamp.
__device__ __forceinline__ float avirhip_x86_round_fix( const float a,
	const float t, const float pk_out )
{
	return( fabsf( a ) >= 2147483648.0f ? ( a < 0.0f ? pk_out : 0.0f ) : t );
}

// Return codes of the kernel families' launchers (the *_run functions below):
// AVIRHIP_OK -- the call's rows are enqueued; an AVIRHIP_E* code -- it failed;
// 1 -- the launcher cannot take THIS call (its pointers' alignment, a source
// window, an element type): nothing was launched and nothing is wrong. There
// is no other private code: api.cpp's road (avir_road, lanc_road) lists the
// attempts of a call up front, makes the buffers of the next one ready and
// goes on to it.

namespace avirhip {

enum { OP_FIR = 0, OP_GATHER = 1, OP_UPF = 2 };
enum { VIEW_CLAMP = 0, VIEW_ZS = 1, VIEW_RAW = 2 };

// One lowered op. All pointers are device pointers owned by the plan.
struct LOp
{
	int type;
	int view;
	int in_len;     // logical input length (clamp range)
	int in_prefix;  // VIEW_RAW: pixels stored before logical index 0
	int zs_mmax;    // VIEW_ZS: source index m > zs_mmax reads 0.0f
	int out_len;    // logical output length
	int out_prefix; // OP_UPF: OutPrefix pixels stored before index 0
	int out_total;  // out_prefix + out_len + suffix (materialised length)

	// OP_FIR: out[n] = f[0]*in[c] + sum_i f[i]*(in[c+i] + in[c-i]),
	// c = rf*(n-e)  (doFilter, avir.h:3748-3866)
	int rf, lat, e;
	float* d_flt; // FIR: &Flt[FltLatency] (lat+1 taps); UPF: whole Flt
	std::vector< float > h_flt;
	// (plan -> f64: the same tables in double, and the float ones stay empty)
	double* d_flt64;
	std::vector< double > h_flt64;

	// OP_GATHER: out[j] = 0 + sum_{t<ntaps[j]} coef[j][t]*in[start[j]+t]
	// (doResize / doResize2, avir.h:3884-4328). coef is pre-expanded per
	// output position: order-0 taps, or ftp[i] + ftp2[i]*x in float.
	int maxtaps;
	int* d_start;
	int* d_ntaps;
	float* d_coef; // [out_len][maxtaps]
	std::vector< int > h_start, h_ntaps;
	std::vector< float > h_coef;
	double* d_coef64;
	std::vector< double > h_coef64;

	// OP_UPF (filtered upsample, avir.h:3404-3733)
	int flen, up_inprefix, up_R, sdc_len, pdc_len, pdc_d0;
	float* d_sdc;
	float* d_pdc;
	double* d_sdc64;
	double* d_pdc64;
};

struct LAxis
{
	std::vector< LOp > ops;
	int src_len, dst_len;
};

// Image element access: address(scan, idx, c) =
//   base + scan*scan_stride + (idx + prefix)*idx_stride + c
template< typename F >
struct Surf
{
	F* base;
	long scan_stride;
	long idx_stride;
	int prefix;
};

struct LancirAxisDev
{
	int kernel_len, src_len, dst_len, n_filters;
	int* d_start;   // [dst_len]: first source pixel, un-padded coordinates
	int* d_fidx;    // [dst_len]
	float* d_flt;   // [n_filters][kernel_len]
	std::vector< int > h_start, h_fidx;
	std::vector< float > h_flt;
};

} // namespace avirhip

struct avirhip_plan
{
	int is_lancir;
	int device;
	int src_w, src_h, src_stride, new_w, new_h, new_stride;
	int ch;    // channels the kernels execute with (4 when 1-3 channel pixels
	           // are padded so that the RGBA fast paths apply)
	int io_ch; // channels of the caller's buffers (ElCountIO)
	int in_type, out_type;
	double tr_mul, pk_out;
	int gamma, alpha_index; // sRGB gamma stages (avir.h:2841-2930, 2982-3068)
	int dither;             // AVIRHIP_DITHER_* (integer outputs only)
	int fp4;                // plan of an fpclass_float4 object (no in-place float output)
	int f64;                // double pipeline (fpclass_def<double>): generic64.hip runs it
	double* packed64;       // its copy of the source, its result, its intermediates
	double* resbuf64;
	std::vector< double* > hbuf64, vbuf64;
	float* errd_line;       // error-diffusion rows handed between row blocks
	float* d_srgb_tbl;      // 256-entry uint8 linearisation table (gamma plans)
	float* d_gthr;          // uint8 gamma output stage as 2 x 256 thresholds
	avirhip::LAxis h, v;
	// LANCIR
	avirhip::LancirAxisDev lv, lh;
	float l_out_mul, l_clamp;
	int l_unity;
	// LANCIR with integer / scaled RGBA I/O: a float RGBA, unity-gain plan of
	// the same geometry whose fast kernels run between a pack pass and the
	// output stage (nullptr: this plan runs its own kernels)
	avirhip_plan* inner;
	int l_order; // LANCIR: channel count whose summation order the kernels use

	int path;       // forced path (0 = auto)
	int variant;    // AVIRHIP_VARIANT_* bits (0 = automatic kernel forms)
	int fused_ok;   // tiled kernels: bit 0 = two-pass (path 2), bit 1 = fused (3)
	int auto_path;  // path taken when `path` == 0
	void* fused;    // tiled-kernel private data
	void* up2;      // exact-2x marching kernel private data (fused_ok bit 2)
	void* lanc2;    // LANCIR exact-2x kernel private data (fused_ok bit 2)
	void* gpass;    // general-ratio pass kernels, path 5 (fused_ok bit 3)
	void* tile64;   // double pipeline: LDS-tiled two-pass executor (tile64.hip)

	// scratch (device), lazily sized
	std::vector< void* > allocs;
	size_t alloc_bytes; // device bytes this plan holds (tables + scratch)
	float* packed;  // source converted to float (non-f32 input)
	float* resbuf;  // float result before the integer / f64 epilogue
	float* lres;    // LANCIR: float result rows before the output stage
	std::vector< float* > hbuf, vbuf; // per-op outputs
	// avirhip_resize_sharded: replicas of this plan on other devices, and the
	// per-replica band / source buffers
	std::vector< avirhip_plan* > replicas;
	// same-device copies used when a call finds this plan's scratch busy
	// (concurrent resizeImage() calls on one object); `is_spare` marks them
	std::vector< avirhip_plan* > spares;
	int is_spare;
	void* shard_band; size_t shard_band_bytes;
	int shard_ldev; // replica: the device id its owner's caller named
	void* shard_src; size_t shard_src_bytes;
	// A plan owns scratch buffers (packed source, float result, FltBuf, op
	// outputs, staging): calls that use them are serialised -- host side by
	// the mutex, device side by making every call's stream wait for the
	// previous call's completion event.
	std::mutex exec_mtx;
	std::mutex shard_mtx; // avirhip_resize_sharded: replicas, band buffers
	std::mutex spare_mtx; // the list of spares
	hipEvent_t last_done;
	void* last_stream; // stream of the last call that used the scratch buffers
	bool last_used;    // (there was one)
	std::thread::id last_tid; // its thread (hipStreamPerThread: one handle, a stream per thread)
	bool last_recorded; // last_done was recorded when that call ended (per-thread streams)
	// host-pointer calls: copy streams and events of the band pipeline
	void* pipe_in; void* pipe_out;
	std::vector< hipEvent_t > pipe_ev;
	void* stage_src; // host-pointer staging
	void* stage_dst;
	size_t stage_src_bytes, stage_dst_bytes;
	std::atomic< void* > avirp; std::mutex avirp_mtx; // avirp.hip's lazy tile tables (see avirp_run)
};

namespace avirhip {

// What belongs to ONE call travels as an argument of that call, from exec_any
// down to the *_run functions, never as state of the plan: plans are shared
// between threads, and some whole-frame calls run without the plan's lock.

// A caller's image as it lies in device memory: element type (AVIRHIP_U8 ...),
// channels per pixel, row pitch in elements. A kernel family that is handed
// one (`raw`, nullptr = none) reads it instead of the float RGBA copy a pack
// pass would make.
struct ImageRef
{
	const void* ptr;
	int type, ch;
	long stride;
};

// The output stage of a LANCIR plan with integer / scaled / 1-3 channel pixels
// (the owner), handed to the kernels of its inner float RGBA plan (`lout`,
// nullptr = none): the last pass applies gain and clamp, converts and stores
// into the owner's image -- `dst` is the band's first row there -- and no float
// result is written. lanc2_run and gpass_run that return 0 for a call with a
// `lout` HAVE stored the owner's pixels: what they cannot store they refuse
// (1).
struct LancirOut
{
	void* dst;
	long stride;
	int type, ch, unity;
	float out_mul, clampv;
};

// avirhip_resize_window on the marching kernels (k_up2, k_lanc2): the source
// pointer handed to them is a VIRTUAL frame base -- window - first rows -- and
// only rows [first, first + rows) exist behind it: the kernels clamp their row
// indices to that range instead of [0, src_h).
// (rows == 0: the whole frame)
struct SrcWindow
{
	int first, rows;
};

void set_error( const char* fmt, ... );
void clear_error();
#define AVIRHIP_HIPCHECK( expr ) do { hipError_t e_ = ( expr ); \
	if( e_ != hipSuccess ) { avirhip::set_error( "%s: %s (%s:%d)", #expr, \
		hipGetErrorString( e_ ), __FILE__, __LINE__ ); \
		return( e_ == hipErrorOutOfMemory ? AVIRHIP_ENOMEM : AVIRHIP_EHIP ); } } \
	while( 0 )

// The boundary is exception-tight (include/avirhip.h, "Conventions"): every
// `extern "C"` entry point is a function-try-block that ends in AVIRHIP_CATCH.
// guard_fail() runs inside the handler, classifies the exception in flight
// (std::bad_alloc -> AVIRHIP_ENOMEM, anything else -> AVIRHIP_EINTERNAL) and
// leaves the message for avirhip_last_error(). The reference's own contract is
// "no exceptions besides bad_alloc" (avir.h:564-827 CBuffer::alloc); the C++
// front end (include/avir_hip) turns AVIRHIP_ENOMEM back into std::bad_alloc.
int guard_fail( const char* fn ) noexcept;
#define AVIRHIP_CATCH( fn ) catch( ... ) { return( avirhip::guard_fail( #fn )); }

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to a loaded function on a
// device, not to a launch: it is raised when a launch needs more dynamic LDS
// than any earlier one asked for, not once per frame (a driver call on the hot
// path otherwise). `have` is the call site's own record, one slot per device.
inline hipError_t ensure_dyn_lds( const void* fn, const size_t bytes,
	std::atomic< int >* have )
{
	int dev = 0;
	(void) hipGetDevice( &dev );
	std::atomic< int >& h = have[ dev & 31 ];

	if( h.load( std::memory_order_relaxed ) >= (int) bytes )
	{
		return( hipSuccess );
	}

	const hipError_t e = hipFuncSetAttribute( fn,
		hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes );

	if( e == hipSuccess )
	{
		h.store( (int) bytes, std::memory_order_relaxed );
	}

	return( e );
}
#define AVIRHIP_DYN_LDS( fn, bytes ) ( [&]() -> hipError_t { \
	static std::atomic< int > have_[ 32 ]; \
	return( avirhip::ensure_dyn_lds( (const void*) ( fn ), ( bytes ), have_ )); }() )

// a * b * c * d without wrapping; false when the product does not fit size_t
bool mul_fits( size_t a, size_t b, size_t c, size_t d, size_t* out = nullptr );
// Geometry every entry point checks before it allocates: row lengths in
// elements fit `int` (the reference computes them in int, avir.h:4786-4794,
// lancir.h:409-411), image sizes in bytes fit size_t. Sets the error string.
bool geometry_ok( const char* fn, int src_w, int src_h, long src_stride,
	int new_w, int new_h, long new_stride, int ch, int in_type, int out_type );

// An owning handle for a plan under construction: a throw between new_plan()
// and the hand-over destroys it (device tables included).
struct PlanHold
{
	avirhip_plan* p;
	explicit PlanHold( avirhip_plan* q ) : p( q ) {}
	~PlanHold();
	avirhip_plan* release() { avirhip_plan* q = p; p = nullptr; return( q ); }
};

size_t dtype_size( int t );

// element types of CImageResizer calls: uint8, uint16, float, double, half,
// bfloat16 (AVIRHIP_U32 is CLancIR's alone)
inline bool avir_dtype_ok( const int t )
{
	return(( t >= AVIRHIP_U8 && t <= AVIRHIP_F64 ) || t == AVIRHIP_F16 ||
		t == AVIRHIP_BF16 );
}

// the 16-bit float types: defined by the float32 call (avirhip.h), planned as
// float32, converted by the pack pass / the output stage or by k_up2 itself
inline bool dtype_is_float16_kind( const int t )
{
	return( t == AVIRHIP_F16 || t == AVIRHIP_BF16 );
}

// The bytes a kernel addresses behind `img` when its rows travel as bytes
// (LDS-DMA: the range check's num_records, an int): `rows` rows at the image's
// pitch, the last one ending with its `width` pixels, rounded up to whole dwords
// (base and pitch are dword-aligned and device allocations dword-granular, so a
// row's last partial dword is fetched whichever way the range check treats a
// dword that straddles the end). 0: no such range -- under a dword, or over
// 0x7ffffffc. (api.cpp's image_bytes is the unrounded size_t of a plan's own
// images, for staging buffers and overlap tests: it stays what it is.)
inline int image_dma_bytes( const ImageRef& img, const int rows,
	const int width )
{
	const long bytes = ( (long) ( rows - 1 ) * img.stride +
		(long) width * img.ch ) * (long) dtype_size( img.type );

	return( bytes >= 4 && bytes <= 0x7ffffffcL ? (int) (( bytes + 3 ) & ~3L ) :
		0 );
}

// The kind of a raw source's elements as the loaders that move rows as bytes
// name it (k_lf's row_px, k_gv's raw_px): 1 uint8, 2 uint16, 3 float, 4 half,
// 5 bfloat16; 0: a type no such loader knows (double, uint32) -- the ONE list
// behind lfuse_takes_raw and gpass_v_raw_ok.
inline int gp_raw_kind( const int t )
{
	return( t == AVIRHIP_U8 ? 1 : t == AVIRHIP_U16 ? 2 : t == AVIRHIP_F32 ? 3 :
		t == AVIRHIP_F16 ? 4 : t == AVIRHIP_BF16 ? 5 : 0 );
}

int finalize_avir_plan( avirhip_plan* p ); // api.cpp
// device bytes a plan holds, with its inner plan, same-device spares and
// other-device replicas (the plan caches' byte bound)
size_t plan_device_bytes( avirhip_plan* p );

// ---- the float and the double tables of one plan, chosen by working type ----

// The tables of an op in the working type F (float, or double for a plan -> f64
// plan), whichever way the op is held: every reader that is written for both
// types -- lowering, upload, the per-op executor -- names them through here.
template< typename V, typename P >
struct OpTab
{
	V h_flt; P d_flt;
	V h_coef; P d_coef;
	P d_sdc; P d_pdc;
};

template< typename F, typename L > // (L: LOp or const LOp)
inline auto op_tab( L& op )
{
	if constexpr( sizeof( F ) == sizeof( double ))
	{
		return( OpTab< decltype(( op.h_flt64 )), decltype(( op.d_flt64 )) >{
			op.h_flt64, op.d_flt64, op.h_coef64, op.d_coef64, op.d_sdc64,
			op.d_pdc64 });
	}
	else
	{
		return( OpTab< decltype(( op.h_flt )), decltype(( op.d_flt )) >{
			op.h_flt, op.d_flt, op.h_coef, op.d_coef, op.d_sdc, op.d_pdc });
	}
}

// The per-op executor's intermediates in the working type F (see op_tab)
template< typename F >
struct PlanBufs
{
	std::vector< F* >& hbuf;
	std::vector< F* >& vbuf;
};

template< typename F >
inline PlanBufs< F > plan_bufs( avirhip_plan* p )
{
	if constexpr( sizeof( F ) == sizeof( double ))
	{
		return( PlanBufs< F >{ p -> hbuf64, p -> vbuf64 });
	}
	else
	{
		return( PlanBufs< F >{ p -> hbuf, p -> vbuf });
	}
}

// generic.hip
// `ch` = channels in `src`, `ech` >= ch = channels written (zero padded)
int launch_pack( const void* src, int in_type, float* dst, int w, int h,
	int ch, int ech, long src_stride, hipStream_t st );
int launch_pack_gamma( const void* src, int in_type, float* dst, int w, int h,
	int ch, int ech, long src_stride, int alpha_index, const float* tbl,
	hipStream_t st );
void srgb_u8_table( float* tbl );
// one lowered op in the working type F (float, double): outputs [idx0, idx1)
// of scanlines [scan0, scan1)
template< typename F >
int launch_op( const LOp& op, int ch, bool x_is_idx, const Surf< F >& in,
	const Surf< F >& out, int scan0, int scan1, int idx0, int idx1,
	hipStream_t st );
int launch_epilogue( const float* res, void* dst, int out_type, long n,
	double tr_mul, double pk_out, int gamma, int ch, int ech,
	int alpha_index, hipStream_t st, const float* gthr = nullptr,
	bool rne = false );
bool gamma_u8_thresholds( float ogm, int use_tr, float trm, float trmi,
	float pk, float* thr );
// the input range [ia, ib] an op reads for outputs [a, b] (api.cpp)
void need_range( const LOp& op, int a, int b, int& ia, int& ib );
// the outputs [va[ i ], vb[ i ]] each op of a plan's vertical chain makes for
// output rows [row0, row1), and the FltBuf rows [ya, yb] the first one reads
struct VRanges
{
	std::vector< int > va, vb;
	int ya, yb;
};
VRanges v_ranges( const LAxis& v, int row0, int row1 ); // api.cpp
// the per-op executor (api.cpp): its intermediates, and the chain of a plan for
// output rows [row0, row1) into `dst` (a surface of F whose row `row0` is at
// dst), float plans in float, plan -> f64 plans in double
template< typename F >
int ensure_generic_scratch( avirhip_plan* p );
template< typename F >
int run_generic( avirhip_plan* p, const F* src, long src_stride, F* dst,
	int row0, int row1, hipStream_t st );
// the source rows [*first, *last] the outputs [row0, row1) of a lowered axis
// read; the same from a plan description's vertical axis (host only)
void axis_src_range( const LAxis& ax, int row0, int row1, int src_len,
	int* first, int* last );
int desc_band_src_rows( const avirhip_plan_desc* d, int row0, int row1,
	int* first, int* last );

// generic64.hip: the double pipeline (plan -> f64), output rows [row0, row1)
int exec_f64( avirhip_plan* p, const void* src, void* dst, int row0, int row1,
	hipStream_t st );

// tile64.hip: the double pipeline's tiled two-pass executor. tile64_run
// returns 1 when the plan has none (filtered upsamples: generic64.hip runs it).
int tile64_prepare( avirhip_plan* p );
void tile64_release( avirhip_plan* p );
bool tile64_ok( const avirhip_plan* p );
int tile64_run( avirhip_plan* p, const void* src, int src_type, long src_ss,
	void* dst, int dst_type, long dst_ss, int row0, int row1, int ya, int yb,
	hipStream_t st );

// up64.hip: marching kernels of the double pipeline's upsizing chains
// (FIR7 -> 12-tap gather over the zero-stuffed view), used by tile64_run for
// the axes that have them; 1: the call was not taken
bool up64_axis_ok( const LAxis& ax );
int up64_run_h( const avirhip_plan* p, const void* src, int src_type,
	long src_ss, double* fltbuf, int ya, int yb, hipStream_t st );
int up64_run_v( const avirhip_plan* p, const double* fltbuf, void* dst,
	int dst_type, long dst_ss, int row0, int row1, hipStream_t st );

int launch_errd( const float* res, void* dst, int out_type, int w, int h,
	int ch, int ech, double tr_mul, double pk_out, int gamma, int alpha_index,
	float* line, hipStream_t st );
int launch_lancir_out( const avirhip_plan* p, const float* res, long rstride,
	void* dst, int nrows, hipStream_t st );
int launch_lancir_out_pad( const avirhip_plan* p, const float* res, void* dst,
	int nrows, hipStream_t st );
int launch_lancir_generic( const avirhip_plan* p, const void* src, void* dst,
	float* tmp, int row0, int row1, hipStream_t st );

// fused.hip
int fused_prepare( avirhip_plan* p );
void fused_release( avirhip_plan* p );
// Runs path `mode` (2 = two-pass tiled, 3 = fused). Returns 1 when the call
// cannot take a tiled path (e.g. unaligned rows) and the generic path should.
// `src_type` / `src_ch`: element type and channel count of the array at `src`
// (AVIRHIP_F32 and 4: a float RGBA image; AVIRHIP_U8 / AVIRHIP_U16 with 1-4
// channels: the caller's integer image, converted and padded by the tile
// loader itself -- no pack pass). `src_stride` in elements of that type.
int fused_run( avirhip_plan* p, int mode, const void* src, int src_type,
	int src_ch, long src_stride, float* dst, int row0, int row1,
	hipStream_t st, void* iout );
bool fused_stores_int( const avirhip_plan* p, int mode );
bool fused_takes_raw( const avirhip_plan* p, int mode );

// dn.hip: integer-ratio downsizing passes used by the two-pass tiled path
int dn_prepare( avirhip_plan* p, void** out );
void dn_release( void* d );
bool dn_has_h( const void* d );
bool dn_has_v( const void* d );
int dn_run_h( void* d, const void* src, int src_type, int src_ch, long src_ss,
	float* flt, long flt_ss, int a, int b, hipStream_t st );
struct GPOut; // gpass_dev.h: the integer output stage fused into a store
int dn_run_v( void* d, const float* flt, long flt_ss, int width, float* dst,
	int row0, int row1, hipStream_t st, const GPOut* out = nullptr );
// dnf.hip: both axes of such a plan in one marching launch (no FltBuf);
// returns 1 when the call cannot take it
int dn_run_hv( void* d, const float* src, long src_ss, float* dst, int row0,
	int row1, hipStream_t st, const GPOut* out = nullptr );
// ... with half / bfloat16 pixels on a side (k_dnfh): RGBA rows of `src` read
// where they lie (half, bfloat16, float), float RGBA rows to `dst` or the
// caller's pixels through `out` (half / bfloat16 narrowed in the store). 1: the
// call is not its own (float on both sides, an image lanc2h_image_ok refuses,
// rows beyond a 32-bit byte offset)
int dn_run_hv16( void* d, const ImageRef& src, float* dst, int row0, int row1,
	hipStream_t st, const GPOut* out );
// fused.hip: whether mode 2 of this plan is the one-launch kernel (both axes
// whole-ratio downsizing, not switched off), and its call with a half /
// bfloat16 image on a side; `iout`: the caller's rows the kernel stores itself
bool fused_dn16( const avirhip_plan* p );
int fused_run_dn16( avirhip_plan* p, const ImageRef& src, float* dst, int row0,
	int row1, hipStream_t st, void* iout );
// ... with sRGB gamma and 8-bit pixels on a side (k_dnfh's DH_S8 kinds): what
// the loader and the store need of the plan beside DnFParams -- the
// linearising table of 256 floats, the 2 x 256 thresholds of the
// de-linearising stage, and the parameters of that stage's direct branch
// (launch_pack_gamma's gm, launch_epilogue's ogm and truncation)
struct DnGamma
{
	const float* tbl; const float* thr;
	int alpha_index, use_tr;
	float gm, ogm, tr_mul, tr_muli, pk_out;
};
// dnf.hip: a uint8 RGBA source read where it lies (`src.type` AVIRHIP_U8; base
// and pitch multiples of 4 bytes) or float RGBA rows; a uint8 result of 1-4
// channels stored bytewise through `out`, or float RGBA rows to `dst`. 1: the
// call is not its own (no 8-bit side, such an image, rows beyond a 32-bit
// byte offset)
int dn_run_hv8( void* d, const ImageRef& src, float* dst, int row0, int row1,
	hipStream_t st, const GPOut* out, const DnGamma& G );
// fused.hip: the call of a gamma plan whose mode 2 is the one-launch kernel
int fused_run_dnsrgb( avirhip_plan* p, const ImageRef& src, float* dst,
	int row0, int row1, hipStream_t st, void* iout );

// gpass.hip: general-ratio pass kernels (path 5), AVIR and LANCIR RGBA float
int gpass_prepare( avirhip_plan* p );
void gpass_release( avirhip_plan* p );
bool gpass_ok( const avirhip_plan* p );
bool gpass_preferred( const avirhip_plan* p );
bool gpass_takes_raw( const avirhip_plan* p );
// whether the pass kernels read and store half / bfloat16 pixels themselves
// (AVIRHIP_GP_NO_IO16, read per call: the pack pass and the output stage)
bool gpass_io16();
// the last source row the first pass of output rows [row0, row1) reads
int gpass_last_src_row( const avirhip_plan* p, int row0, int row1 );
bool gpass_lancir_takes_raw( const avirhip_plan* p, const ImageRef& raw );
// `raw`: the image the first pass reads instead of `src`; `iout`: the last pass
// of an AVIR plan stores the caller's pixels there; `lout`: the last pass of a
// LANCIR inner plan runs its owner's output stage
int gpass_run( avirhip_plan* p, const float* src, long src_stride, float* dst,
	int row0, int row1, hipStream_t st, const ImageRef* raw, void* iout,
	const LancirOut* lout );
bool fused_dn_both( const avirhip_plan* p );

// up2.hip: specialised exact-2x RGBA kernel (path 4)
int up2_prepare( avirhip_plan* p );
void up2_release( avirhip_plan* p );
int up2_run( avirhip_plan* p, const float* src, long src_stride, float* dst,
	int row0, int row1, hipStream_t st, SrcWindow win, const ImageRef* raw,
	void* iout );
bool up2_stores_io( const avirhip_plan* p );
// whether up2_run / lanc2_run take this float RGBA call for certain (no refusal,
// no fall-back to kernels that know nothing of a source window)
bool up2_takes_window( const avirhip_plan* p, const void* src, const void* dst );
bool lanc2_takes_window( const avirhip_plan* p, const void* src, const void* dst );

// lanc2.hip: LANCIR exact-2x RGBA float kernel (path 4 of LANCIR plans)
int lanc2_prepare( avirhip_plan* p );
void lanc2_release( avirhip_plan* p );
int lanc2_run( const avirhip_plan* p, const float* src, float* dst, int row0,
	int row1, hipStream_t st, SrcWindow win, const ImageRef* raw,
	const LancirOut* lout );
bool lanc2_takes_raw( const avirhip_plan* q, const ImageRef& raw );
const float* lanc2_coef( const avirhip_plan* p );

// lanc2h.hip: LANCIR exact-2x RGBA with half / bfloat16 images on either side,
// one launch over the images where they lie (`q`: the inner float RGBA plan).
// lanc2h_image_ok: what the kernel asks of an image (a pixel naturally
// aligned; `stride` in elements); lanc2h_run returns 1 for a call that is not
// its own (float on both sides, an image the predicate refuses).
bool lanc2h_image_ok( const void* ptr, int type, long stride );
int lanc2h_run( const avirhip_plan* q, const ImageRef& src,
	const LancirOut& out, int row0, int row1, hipStream_t st );

// pviews.hip: plane views (include/avirhip.h, "Plane views"). One plane of a
// planar call as k_lancp / k_avirp read it from their table: where the source
// and the result plane lie, pitches and element strides in BYTES.
struct PlaneViewDev
{
	const char* src; long src_pb, src_eb;
	char* dst; long dst_pb, dst_eb;
};

typedef std::vector< PlaneViewDev > PlaneViewTable;

// The way of a call's table to the device: a slot of a process-wide pool (a
// pinned host buffer, a device buffer, an event) is taken under the pool's
// mutex, which is held for the search alone; the table is copied into the
// pinned buffer -- the caller's array is free from then on -- and from there to
// the device buffer on the call's stream; done() records the slot's event
// behind the launch and hands the slot back, to be taken again once the event
// has passed. No call waits for the device, no two calls share a buffer, no
// plan owns one: calls on one plan from several threads stay lock-free.
class PlaneViewUpload
{
public:
	PlaneViewUpload() : slot( nullptr ), pushed( nullptr ) {}
	~PlaneViewUpload(); // a call that failed behind push(): done() on its stream
	int push( const PlaneViewTable& t, int device, hipStream_t st );
	const PlaneViewDev* dev() const;
	void done( hipStream_t st );

private:
	void* slot;
	hipStream_t pushed;
};

// Loads and stores of the VIEWS kernels: a base read from the table is a
// generic pointer to the compiler (flat_load / flat_store, which count with
// the LDS traffic); it is device memory by contract, and said so here
// (global_load / global_store). G false: the plain access of the dense forms,
// whose bases are kernel arguments and global already.
#if defined( __HIPCC__ )
template< bool G, typename T >
__device__ __forceinline__ T pview_load( const char* const p )
{
	if constexpr( G )
	{
		return( *(const __attribute__(( address_space( 1 ))) T*) p );
	}
	else
	{
		return( *(const T*) p );
	}
}

template< bool G, typename T >
__device__ __forceinline__ void pview_store( char* const p, const T v )
{
	if constexpr( G )
	{
		*(__attribute__(( address_space( 1 ))) T*) p = v;
	}
	else
	{
		*(T*) p = v;
	}
}
#endif

// strided <-> tight copy of ONE plane in elements of `es` bytes (1, 2, 4, 8):
// element (r, c) goes from src + r * s_pb + c * s_eb to dst + r * d_pb +
// c * d_eb; nothing else is written. The gather and the scatter of the
// per-plane road of views.
int pview_copy( const void* src, long s_pb, long s_eb, void* dst, long d_pb,
	long d_eb, int w, int h, int es, hipStream_t st );

// lancp.hip: the planes of a CLancIR plan of one channel (avirhip_resize_planes)
// in one launch, one float per lane: `n_planes` source planes `src_ps` elements
// apart, their results `dst_ps` elements apart, rows at the plan's pitches,
// device memory. 1: the call is not its own (an element type outside uint8,
// uint16, float, half, bfloat16; a base that is no multiple of the element
// size; a tile of intermediate rows that exceeds its LDS) and `*why` names
// what it missed; the caller runs the plan's own road per plane. `views`
// (host, validated, or nullptr): every plane where its entry says instead.
int lancp_run( const avirhip_plan* p, const void* src, void* dst, long src_ps,
	long dst_ps, int n_planes, hipStream_t st, const char** why,
	const PlaneViewTable* views = nullptr );

// avirp.hip: the same for a CImageResizer plan of one channel -- k_avirp runs
// the plan's lowered ops of both axes on LDS tiles, all planes in one launch.
// 1: the call is not its own (float64 elements; gamma, error-diffusion,
// fpclass_float4 and double plans; a base that is no multiple of the element
// size; a chain of more than three ops; no tile within its LDS) and `*why`
// names what it missed. avirp_release frees what the first call made.
int avirp_run( avirhip_plan* p, const void* src, void* dst, long src_ps,
	long dst_ps, int n_planes, hipStream_t st, const char** why,
	const PlaneViewTable* views = nullptr );
void avirp_release( avirhip_plan* p );

} // namespace avirhip
