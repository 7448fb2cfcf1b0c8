/*
 * avirhip.h -- C ABI of libavirhip: the MI355X (gfx950) executor for the
 * separable-resize hot path of avaneev/avir.
 *
 * The reference (header-only C++, /root/reference) has no FFI of its own; its
 * extension point for this path is the `fpclass` template parameter
 * (avir.h:4569-4592), a per-scanline interface. This header is the boundary a
 * drop-in replacement binds instead: the reference's front-end
 * (avir::CImageResizer<>::resizeImage, avir.h:4680-4684; avir::CLancIR::
 * resizeImage, lancir.h:386-390) keeps its signature, runs the planner on the
 * host, and hands the immutable plan + the two image buffers across this ABI.
 * See INTEGRATION.md for the reference-side stub.
 *
 * Conventions: plain C, plain pointers and sizes. Every function returning
 * `int` returns 0 on success and a negative AVIRHIP_E* code on error;
 * avirhip_last_error() returns a thread-local message. No C++ exception
 * crosses the boundary: every entry point is a function-try-block, a failed
 * host allocation comes back as AVIRHIP_ENOMEM (a failed device allocation as
 * AVIRHIP_EHIP / AVIRHIP_ENOMEM), anything else as AVIRHIP_EINTERNAL, and the
 * object the call worked on stays usable. Image geometries whose element or
 * byte counts do not fit the reference's own `int` / `size_t` arithmetic
 * (avir.h:4786-4794, lancir.h:409-430) are refused with AVIRHIP_EINVAL before
 * anything is allocated. The library copies every table it is given; the
 * caller keeps ownership of its arrays.
 */
#ifndef AVIRHIP_H
#define AVIRHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVIRHIP_OK 0
#define AVIRHIP_EINVAL (-1)      /* bad argument / malformed plan */
#define AVIRHIP_ENODEV (-2)      /* no usable gfx950 device */
#define AVIRHIP_EHIP (-3)        /* HIP runtime error (see last_error) */
#define AVIRHIP_EUNSUPPORTED (-4)/* valid request outside the built scope */
#define AVIRHIP_ENOMEM (-5)       /* host or device memory exhausted */
#define AVIRHIP_EINTERNAL (-6)    /* an unexpected C++ exception was caught at the
                                     boundary (never crosses it; see last_error) */

/* Element types of the source / destination image (Tin/Tout of
 * resizeImage<Tin,Tout>, avir.h:4670-4677; lancir.h:373-381). */
typedef enum avirhip_dtype {
	AVIRHIP_U8 = 0,
	AVIRHIP_U16 = 1,
	AVIRHIP_F32 = 2,
	AVIRHIP_F64 = 3,
	/* CLancIR only: 32-bit unsigned elements whose value range is treated as
	 * uint16_t's, 0..65535 (lancir.h:373-377; Clamp / OutMul derive from
	 * sizeof() == 1 or not, lancir.h:531-533). */
	AVIRHIP_U32 = 4,
	/* IEEE binary16 ("half") elements. The reference has no such type; a call
	 * with half elements is DEFINED by the same call with float buffers.
	 * Source: every half (denormals included) is widened exactly to float, and
	 * the call then behaves in every respect as a float32 source does (scaling,
	 * SrcBitDepth, gamma linearisation, channel padding). Result: the call
	 * computes exactly the float32 result fpclass_def<float> / CLancIR would
	 * store into a float32 destination (with UseSRGBGamma it stays linear; no
	 * clamp, no PkOut scale, not dithered), and each element is narrowed to
	 * half with round-to-nearest-even: half denormals are kept, values beyond
	 * +-65504 become +-Inf, NaN stays NaN. The two sides are independent: half
	 * mixes freely with the other types. fpclass_float4 and fpclass_def<double>
	 * refuse half elements (AVIRHIP_EUNSUPPORTED): their float results pass
	 * through an output stage of their own -- a different contract.
 * (Three kernels read and store half RGBA pixels themselves, one launch over
 * the caller's images: CImageResizer's exact-2x marching kernel k_up2, its
 * whole-ratio (2x, 3x) downsizing kernel k_dnfh, and CLancIR's exact-2x kernel
 * k_lanc2h. At any other ratio CImageResizer's pass kernels do, for pixels of
 * 1-4 channels: k_gh reads a half source where it lies, and so do the
 * accumulation kernels k_sacc / k_sacc2 where the horizontal axis downsizes by
 * 2 or more and the frame has 65,536 pixels or more (any row pitch, a base
 * that is a multiple of 2); the last pass -- k_gv, k_gf, k_sacc* -- narrows
 * and stores a half result; smaller frames of such an axis, k_gf and k_gh2
 * read the pack pass's float copy of the source. From 3,600,000 source pixels
 * on, such a downsizing call takes these kernels by itself, without a float
 * copy of either image. CLancIR's pass kernels do the same at its other
 * ratios, 1-4 channels: k_lf (upsizing, one launch) and k_gv read a half
 * source where it lies -- dword-aligned base and row pitch, more than 48
 * columns, up to 24 taps -- and k_lf / k_gh apply the gain, narrow and store a
 * half result at any even address; an image they cannot take goes through
 * the pack pass / the output stage with the same bits. Everywhere else -- the
 * tiles, gamma, CLancIR's exact-2x calls with 1-3 channels or an integer
 * result behind a half source, its generic kernels -- the pack pass widens
 * and the output stage narrows.)
 * (8-bit images with UseSRGBGamma: whole-ratio (2x, 3x) downsizing on both
 * axes runs in one launch of k_dnfh as well, with the reference's bits. It
 * linearises a uint8 RGBA source where it lies -- a base and a row pitch that
 * are multiples of 4 bytes -- and de-linearises and stores a uint8 result of
 * 1-4 channels itself, at any address (the default ditherer). The sides are
 * independent: any other source (RGB, uint16, float, an image that misses the
 * modulus) goes through the pack pass first -- and keeps the kernel's store
 * for frames of up to 1,000,000 source pixels, the output stage beyond -- any
 * other result through float rows and the output stage;
 * AVIRHIP_VARIANT_DN_UNFUSED_IO keeps both stages.
 * Every other gamma call takes the pack pass and the output stage.) */
	AVIRHIP_F16 = 5,
	/* bfloat16 elements: 16 bits holding the upper half of an IEEE binary32.
	 * A call with bfloat16 elements is DEFINED by the same call with float
	 * buffers, as AVIRHIP_F16's is. Source: each element is widened exactly,
	 * float bits = element bits << 16, for every bit pattern (denormals
	 * included; a NaN stays a NaN), and the call then behaves in every respect
	 * as a float32 source does (scaling, SrcBitDepth, gamma linearisation,
	 * channel padding). Result: the call computes exactly the float32 result
	 * fpclass_def<float> / CLancIR would store into a float32 destination (with
	 * UseSRGBGamma it stays linear; no clamp, no PkOut scale, not dithered), and
	 * each element u (float bits) is narrowed round-to-nearest-even:
	 * ( u + 0x7fff + (( u >> 16 ) & 1 )) >> 16 for every non-NaN u -- float32
	 * denormals become bfloat16 denormals, values that round beyond the largest
	 * finite bfloat16 become +-Inf; a NaN becomes a NaN of unspecified payload
	 * and sign. The two sides are independent: bfloat16 mixes freely with every
	 * other type, AVIRHIP_F16 included. fpclass_float4 and fpclass_def<double>
	 * refuse bfloat16 elements (AVIRHIP_EUNSUPPORTED) as they refuse half ones;
	 * CLancIR accepts them on either side under the same rule. (k_up2, k_dnfh
 * and k_lanc2h read and store bfloat16 RGBA pixels themselves, as they do
 * half ones, and so do the pass kernels -- k_gh and k_sacc / k_sacc2 the
 * source, k_gv / k_gf / k_sacc* the result, 1-4 channels, under the same
 * conditions as for half -- at every other ratio, and CLancIR's:
 * k_lf / k_gv the source, k_lf / k_gh the result.) */
	AVIRHIP_BF16 = 6
} avirhip_dtype;

/* Whether the compiler has the `__bf16` storage type (the C++ front ends map
 * it to AVIRHIP_BF16). g++ (13 and later) announces it with
 * __BFLT16_MANT_DIG__; clang predefines no macro for it, so there the test is
 * the version that brought the type to the target: x86 with SSE2, AArch64,
 * AMDGPU. (Of these, the tests build with the HIP toolchain's clang on x86
 * alone.) */
#if defined( __BFLT16_MANT_DIG__ ) || ( defined( __clang__ ) && \
	__clang_major__ >= 15 && ( defined( __SSE2__ ) || defined( __aarch64__ ) || \
	defined( __AMDGPU__ )))
#define AVIRHIP_HAS_BF16 1
#endif

/* Where a buffer passed to an execute call lives. */
#define AVIRHIP_MEM_HOST 0
#define AVIRHIP_MEM_DEVICE 1
#define AVIRHIP_MEM_AUTO 2 /* ask the HIP runtime (hipPointerGetAttributes) */
/* Planar calls only: `src` / `dst` is a HOST array of n_planes
 * avirhip_plane_view, one per plane ("Plane views" below). */
#define AVIRHIP_MEM_VIEWS 3
#define AVIRHIP_HAS_VIEWS 1

/* One plane of a planar call where it lies in DEVICE memory: element (r, c) of
 * the plane is base[ r * row_pitch + c * elem_stride ], in elements of the
 * side's type. */
typedef struct avirhip_plane_view {
	void*     base;        /* device pointer to element (0,0) of the plane */
	long long row_pitch;   /* elements between rows; 0: the call's own rule */
	long long elem_stride; /* elements between neighbours in a row; 0 or 1: dense */
} avirhip_plane_view;      /* 24 bytes */

/* ---------------------------------------------------------------------
 * AVIR plan description: a faithful, flattened mirror of the reference's
 * per-axis filtering-step list (CImageResizerFilterStep, avir.h:2568-2728)
 * after buildFilterSteps / updateFilterStepBuffers / updateBufLenAndRPosPtrs
 * (avir.h:5616-6127) have run.
 * ------------------------------------------------------------------- */

typedef enum avirhip_step_kind {
	AVIRHIP_STEP_FIR = 0,          /* doFilter, avir.h:3748-3866 */
	AVIRHIP_STEP_UP_ZEROSTUFF = 1, /* doUpsample, FltOrig kept, 3260-3402 */
	AVIRHIP_STEP_UP_FILTERED = 2,  /* doUpsample with filter + DC tails, 3404-3733 */
	AVIRHIP_STEP_RESIZE = 3,       /* doResize, avir.h:3884-4096 */
	AVIRHIP_STEP_RESIZE2 = 4       /* doResize2, avir.h:4114-4328 */
} avirhip_step_kind;

/* One entry of the resizing-position table (CResizePos, avir.h:2640-2648;
 * filled by fillRPosBuf 5782-5808 and updateBufLenAndRPosPtrs 6063-6126). */
typedef struct avirhip_rpos {
	int32_t src_pos_int; /* floor(o + k*j) */
	int32_t fti;         /* fractional-delay filter index */
	int32_t phase;       /* index of `fti` in the step's compact phase list */
	float x;             /* order-1 interpolation coefficient (float) */
	int32_t src_offs_px; /* SrcOffs / ElCount: first source pixel read */
	int32_t fl;          /* taps walked (RESIZE2: FilterLen - fo, step 2) */
	int32_t ftp_off;     /* fo: offset of the first tap inside the phase */
	double x64;          /* double pipeline: the coefficient in double (x unused) */
} avirhip_rpos;

typedef struct avirhip_step {
	int32_t kind;            /* avirhip_step_kind */
	int32_t resample_factor; /* ResampleFactor (0 for RESIZE/RESIZE2) */
	int32_t in_len, in_prefix, in_suffix;
	int32_t out_len, out_prefix, out_suffix;
	int32_t edge_pixel_count;

	/* FIR / UP_FILTERED: the step's filter (Flt) and latency. Unused (len 0)
	 * for UP_ZEROSTUFF and RESIZE*. */
	int32_t flt_len;
	int32_t flt_latency;
	const float* flt;
	/* UP_FILTERED only: PrefixDC / SuffixDC tails (avir.h:5307-5353). */
	int32_t prefix_dc_len;
	const float* prefix_dc;
	int32_t suffix_dc_len;
	const float* suffix_dc;

	/* RESIZE / RESIZE2: the fractional-delay bank, compacted to the phases
	 * the position table references. Phase p holds `bank_filter_len`
	 * order-0 taps followed (order 1 only) by `bank_filter_len` difference
	 * taps (avir.h:1838-1841). */
	int32_t bank_filter_len;
	int32_t bank_order;      /* 0 or 1 */
	int32_t bank_frac_count; /* FracCount of the full bank */
	int32_t n_phases;
	const int32_t* phase_fti; /* [n_phases], ascending */
	const float* phase_taps;  /* [n_phases][filter_len * (order + 1)] */
	const avirhip_rpos* rpos; /* [out_len] */

	/* Double pipeline (avirhip_plan_desc::work_f64, the reference's
	 * fpclass_def<double>): the same tables in double precision -- the
	 * float fields above are null then, and rpos[].x64 replaces rpos[].x. */
	const double* flt64;
	const double* prefix_dc64;
	const double* suffix_dc64;
	const double* phase_taps64;
} avirhip_step;

typedef struct avirhip_axis {
	int32_t n_steps;
	const avirhip_step* steps;
	int32_t build_mode; /* informational: the mode the planner selected */
} avirhip_axis;

typedef struct avirhip_plan_desc {
	int32_t src_w, src_h;
	int32_t src_stride_elems; /* SrcScanlineSize (elements); <1 => w*ch */
	int32_t new_w, new_h;
	int32_t channels;         /* ElCountIO, 1..4 */
	int32_t in_type, out_type;/* avirhip_dtype */
	avirhip_axis h;           /* horizontal pass: src rows -> FltBuf */
	avirhip_axis v;           /* vertical pass: FltBuf columns -> result */
	/* Integer-output epilogue (avir.h:5029-5045, 4392-4419). Ignored for
	 * float/double output. */
	double tr_mul;            /* TrMul (1.0: no bit-depth truncation) */
	double pk_out;            /* PkOut: 255 or 65535 */
	/* sRGB gamma (CImageResizerVars::UseSRGBGamma / AlphaIndex, avir.h:2526-2527):
	 * the source is linearised while it is packed (packScanline gamma branch,
	 * avir.h:2841-2930, convertSRGB2Lin 206-291) and the result de-linearised
	 * before the dither/unpack stage (applySRGBGamma, avir.h:2982-3068,
	 * convertLin2SRGB 301-312); the alpha channel (index 0 or 3 of 4-channel
	 * pixels, -1 = none) is only scaled. As in the reference, float32 output
	 * is the vertical pass' in-place result and stays linear (avir.h:4956-4979). */
	int32_t use_srgb_gamma;
	int32_t alpha_index;
	/* Ditherer of the integer-output stage -- the reference selects it with
	 * the third template parameter of fpclass_def (avir.h:4569-4592):
	 * AVIRHIP_DITHER_DEF = CImageResizerDithererDefINL (round + clamp,
	 * avir.h:4351-4427), AVIRHIP_DITHER_ERRD = CImageResizerDithererErrdINL
	 * (error diffusion along and across rows, avir.h:4441-4537; "recursive":
	 * rows depend on each other, so such a plan cannot execute row bands). */
	int32_t dither;
	/* 1: the double pipeline (the reference's fpclass_def<double>,
	 * avir.h:4553-4560): tables in the steps' ...64 fields, every pass computes
	 * in double. 0: float (fpclass_def<float>, fpclass_float4). */
	int32_t work_f64;
} avirhip_plan_desc;

#define AVIRHIP_DITHER_DEF 0
#define AVIRHIP_DITHER_ERRD 1
/* CImageResizerDithererDefINL over the SSE value type of fpclass_float4: its
 * round() is cvtps_epi32 under nearest-even (avir_float4_sse.h:303-313)
 * instead of avir::round's (int)(d + 0.5) (avir.h:130-135). Such a plan also
 * has no in-place float output (avir.h:4956: sizeof(fptype) != sizeof(Tout)),
 * i.e. float / double results pass through the output stage, and with sRGB
 * gamma they ARE de-linearised. */
#define AVIRHIP_DITHER_DEF_RNE 2

/* ---------------------------------------------------------------------
 * LANCIR plan description (CLancIR internals, lancir.h:840-1381).
 * ------------------------------------------------------------------- */

typedef struct avirhip_lancir_pos {
	int32_t flt_index; /* index into the axis' `filters` array */
	int32_t so;        /* first source pixel read, relative to the padded
	                      scanline start (CResizePos::so, lancir.h:1231) */
} avirhip_lancir_pos;

typedef struct avirhip_lancir_axis {
	int32_t kernel_len;       /* KernelLen, even */
	int32_t padl, padr;       /* CResizeScanline::padl/padr */
	int32_t src_len, dst_len;
	int32_t n_filters;
	const int32_t* filter_frac; /* [n_filters] phase index 0..1000 */
	const float* filters;       /* [n_filters][kernel_len], un-replicated */
	const avirhip_lancir_pos* pos; /* [dst_len] */
} avirhip_lancir_axis;

typedef struct avirhip_lancir_desc {
	int32_t src_w, src_h, src_stride_elems;
	int32_t new_w, new_h, new_stride_elems;
	int32_t channels;
	int32_t in_type, out_type;
	avirhip_lancir_axis v; /* vertical pass runs first (lancir.h:601-646) */
	avirhip_lancir_axis h;
	float out_mul;         /* OutMul, lancir.h:532-533 */
	float clamp;           /* Clamp, lancir.h:531 */
	int32_t is_unity_mul;  /* IsUnityMul, lancir.h:528-529 */
} avirhip_lancir_desc;

/* ---------------------------------------------------------------------
 * Device / plan / execute.
 * ------------------------------------------------------------------- */

typedef struct avirhip_plan avirhip_plan;

/* Number of usable gfx950 devices (0 when there is none). */
int avirhip_device_count(void);
/* Binds the calling thread to `device` (hipSetDevice). */
int avirhip_init(int device);
/* Thread-local message of the calling thread's most recent avirhip_* call that
 * returns a status: every such entry point empties it when it begins, so the
 * text never outlives the call it describes ("" after a call that succeeded). */
const char* avirhip_last_error(void);
/* Library version string. */
const char* avirhip_version(void);

/* Uploads an AVIR plan to the current device. The plan is immutable and may
 * be shared by threads: executions that need the plan's scratch buffers are
 * serialised inside the library (a mutex on the host side, an event chain on
 * the device side); device-resident float RGBA calls of the single-launch 2x
 * kernels need no scratch and run concurrently. */
int avirhip_plan_create(const avirhip_plan_desc* desc, avirhip_plan** out);
int avirhip_lancir_plan_create(const avirhip_lancir_desc* desc,
	avirhip_plan** out);
void avirhip_plan_destroy(avirhip_plan* plan);

/* Plan tuning: force an execution path, for testing and A/B benchmarking.
 * 0 = automatic (fastest applicable), 1 = generic per-step kernels (every
 * plan), 2 = LDS-tiled two-pass kernels, 3 = LDS-tiled fused single launch,
 * 4 = specialised exact-2x RGBA marching kernel (single launch), 5 = the
 * general-ratio pass kernels (one launch per axis, autonomous wavefronts).
 * Returns AVIRHIP_EUNSUPPORTED if the path cannot run this plan. */
int avirhip_plan_set_path(avirhip_plan* plan, int path);
/* The path the next execution will take (1..5). */
int avirhip_plan_get_path(const avirhip_plan* plan);

/* Kernel variants inside a path, for differential tests and A/B timing (every
 * variant is bit-identical). `variant` is a bit mask, 0 = the automatic choice:
 * AVIRHIP_VARIANT_UP2_PLAIN_V   path 4 runs the 13-row-window form of the
 *     vertical phase (the form a plan whose 2x bank phase is not bit-symmetric
 *     takes) instead of the transposed, product-sharing one;
 * AVIRHIP_VARIANT_DN_TWO_PASS   integer-ratio downsizing (k = 2, 3) runs its
 *     two pass kernels through FltBuf instead of the single fused launch;
 * AVIRHIP_VARIANT_SACC_LADDER   the streaming-accumulation kernel of
 *     downsizing axes runs its general form (one branch per alive output, the
 *     form float sources take) where the branch-free form for integer sources
 *     would run. */
#define AVIRHIP_VARIANT_UP2_PLAIN_V 1
#define AVIRHIP_VARIANT_DN_TWO_PASS 2
#define AVIRHIP_VARIANT_SACC_LADDER 4
/* upsizing on both axes (path 5): the horizontal and the vertical pass kernel
 * through FltBuf instead of the single fused launch of gfuse.hip */
#define AVIRHIP_VARIANT_UPG_TWO_PASS 8
/* ... and the fused launch whatever the frame size (automatically: frames of
 * 7 Mpixels of output and more; CLancIR plans with integer results: up to
 * about 3x horizontally). (The fused kernel k_gf reads float RGBA rows only:
 * a half / bfloat16 source has the pack pass in front of it, a half / bfloat16
 * result is narrowed and stored by it. With AVIRHIP_VARIANT_UPG_TWO_PASS k_gh
 * reads such a source where it lies. The environment variable
 * AVIRHIP_GP_NO_IO16, read per call, puts the pack pass and the output stage
 * around the pass kernels for every half / bfloat16 image, CLancIR's
 * included: A/B timing and differential tests.) */
#define AVIRHIP_VARIANT_UPG_FUSED 16
/* float RGBA sources on downsizing axes: the branch-free accumulation kernels
 * run optimistically (exact kernels behind an alarm) as they do for float
 * pixels of 1-3 channels; automatically such sources take the exact kernels
 * alone, which are as fast there and need no alarm launches */
#define AVIRHIP_VARIANT_SACC_OPTIMISTIC 32
/* path 4: the marching kernel reads the pack pass' float copy of the source and
 * writes a float result for the output stage, where it would read or store the
 * caller's integer / half / bfloat16 pixels itself (the A/B and differential form of the
 * fused I/O; float RGBA images are the kernel's own format either way).
 * With UseSRGBGamma and a uint8 result: the gamma pack pass, the float kernel
 * and the de-linearising output stage, where the kernel would linearise a
 * uint8 RGB / RGBA source and de-linearise and store the result itself (frames
 * of AVIRHIP_UP2SRGB_RAW_MINPIX to AVIRHIP_UP2SRGB_RAW_MAXPIX source pixels,
 * 1,700,000 to 2,700,000 unless set; the store alone up to
 * AVIRHIP_UP2SRGB_STORE_MAXPIX, 0 unless set: environment, read per call).
 * On a CLancIR plan: the pack pass and the output stage always run, whatever
 * the path -- no kernel reads the caller's image as it lies and none stores the
 * caller's pixels itself (AVIRHIP_NO_FUSED_OUT for this plan alone) */
#define AVIRHIP_VARIANT_UP2_UNFUSED_IO 64
/* path 2, whole-ratio downsizing on both axes with half / bfloat16 pixels on a
 * side: the pack pass, k_dnf and the output stage run (two float copies on the
 * plan) where k_dnfh would read and store the caller's 16-bit pixels in its
 * one launch (the A/B and differential form of that kernel) */
#define AVIRHIP_VARIANT_DN_UNFUSED_IO 128
int avirhip_plan_set_variant(avirhip_plan* plan, int variant);

/* Device memory the plan holds right now, in bytes: tables, scratch buffers
 * (allocated when a path first needs them), its inner plan, spares and
 * replicas -- what the front ends' plan caches count against their bound. */
unsigned long long avirhip_plan_device_bytes(avirhip_plan* plan);

/* Executes H pass + V pass (+ integer epilogue) of `plan`:
 * src -> dst. `src_mem`/`dst_mem` are AVIRHIP_MEM_HOST or _DEVICE; host
 * buffers are staged through device memory inside the call. `stream` is a
 * hipStream_t (NULL = default stream). With device buffers the call is
 * asynchronous with respect to the host.
 * Alignment of the images (this call, avirhip_resize_band and
 * avirhip_resize_window alike): any base that is a multiple of the element
 * size, and any source row pitch of at least src_w * channels elements, is
 * served with the reference's bits on the automatic path, and nothing outside
 * the destination's rows is written (CLancIR: nothing between them either).
 * The fast kernels ask more -- 16-byte float RGBA rows, dword-aligned integer
 * rows where they travel as bytes, a dword base for fused uint8 RGBA stores:
 * DESIGN.md section 4e has the table, family by family, with the predicate
 * that says so. A call that misses it steps aside to the pack pass, to a float
 * result and the output stage, or to the generic kernels; a plan forced onto a
 * path (avirhip_plan_set_path) whose kernel has no such stage refuses the call
 * with AVIRHIP_EUNSUPPORTED and stores nothing. tests/test_gpu_align.py stands
 * every kernel family on both sides of each of these. Bases that are no
 * multiple of the element size are served where the half / bfloat16 suites
 * pin that (the pack pass and the output stage take them); for the other
 * element types no test stands there (tests/align_cases.py: LEFT_OUT). */
int avirhip_resize(avirhip_plan* plan, const void* src, int src_mem,
	void* dst, int dst_mem, void* stream);

/* Row-band execution: computes only output rows [row0, row1) of the plan's
 * destination image into `dst_band` (tightly packed band of row1-row0 rows).
 * The source is the WHOLE source image (device or host). Used for multi-GPU
 * sharding: bands computed on different devices are bit-identical to the
 * corresponding rows of a full avirhip_resize(). */
int avirhip_resize_band(avirhip_plan* plan, const void* src, int src_mem,
	void* dst_band, int dst_mem, int row0, int row1, void* stream);

/* The source rows [*first, *last] (inclusive) that output rows [row0, row1)
 * read -- the reference's vertical windows with their replicated edges folded
 * in (avir.h:6560-6619 resizeScanlineV over FltBuf columns; lancir.h:560-640).
 * No other row of `src` influences the band (tools/fuzz_values.py poisons them
 * with NaNs): a caller that streams the source -- row bands of a frame arriving
 * over a link, tiles of a larger image -- only has to have these rows in place
 * when it makes the call. `src` must still address a whole, mapped frame: the
 * marching kernels start their chunks at chunk-aligned rows and may LOAD rows
 * outside the range (their results are discarded, never stored). A caller that
 * holds only the window passes avirhip_resize_window() its rows instead. */
int avirhip_band_source_rows(const avirhip_plan* plan, int row0, int row1,
	int* first, int* last);

/* Row-band execution from a WINDOW of the source: `src_rows` holds only the
 * source rows [first_row, first_row + n_rows) (same row pitch as the plan's
 * source), which must cover avirhip_band_source_rows(row0, row1) -- otherwise
 * AVIRHIP_EINVAL. This is the multi-GPU distribution of SURVEY.md 8(e): rank g
 * receives its band's rows plus the halo and nothing else (the reference's
 * analogue: scanlines dealt to worker threads, avir.h:4885-4890, 4967-4971);
 * image borders are the frame's, never the window's, so the band is
 * bit-identical to the same rows of avirhip_resize(). No other source byte
 * moves, and for the plans the sharded configurations run -- exact 2x, float
 * RGBA in and out: the marching kernels k_up2 / k_lanc2 -- the plan holds
 * O(window) device memory: a DEVICE window is read where it lies (no staging,
 * no copy; nothing outside [src_rows, src_rows + n_rows rows) is touched -- the
 * kernels clamp their row indices to the window, which for every access that
 * reaches a result is the frame's own edge replication), a HOST window is
 * uploaded into a window-sized staging buffer. Other plans copy the window to
 * its place in a frame-sized staging buffer of the plan (their kernels index
 * the frame; what they load outside the window never reaches a result:
 * tests/test_gpu_window.py runs every kernel family from windows whose
 * surroundings -- the rest of that buffer included -- are NaNs / complemented
 * pixels, against the reference's bits).
 * A DEVICE window may share bytes with `dst_band`: the window is then copied
 * aside before anything is stored (into the window-sized staging buffer on the
 * marching kernels), and the band is the same as from a disjoint window.
 * The window is an argument of the call, not state of the plan: window calls,
 * whole-frame calls and band calls of one plan may run on different threads at
 * the same time (avirhip_plan_create). */
int avirhip_resize_window(avirhip_plan* plan, const void* src_rows,
	int src_mem, int first_row, int n_rows, void* dst_band, int dst_mem,
	int row0, int row1, void* stream);

/* One frame sharded over several devices of THIS process:
 * the destination rows are split into `n_gpus` contiguous bands, band g is
 * computed on device `devices[g]` (a replica of the plan is created there on
 * first use; `devices` == NULL or repeated entries run the bands one after
 * another on the same device) and the bands are stitched into `dst` -- peer
 * copies over xGMI when `dst` is device memory, device-to-host copies
 * otherwise. `src`/`dst` are whole images, host or device memory (detected).
 * The stitched frame is bit-identical to avirhip_resize(). `gather_root` is
 * the index of the band whose device should hold `dst` when the caller
 * allocates it there (informational; `dst` is used where it is). The two
 * optional outputs receive the wall time of the compute and gather phases.
 * The multi-PROCESS form of the same sharding (one process per GPU, RCCL) is
 * avirhip_resize_band + avir_amd/sharding.py. */
int avirhip_resize_sharded(avirhip_plan* plan, int n_gpus, const int* devices,
	const void* src, void* dst, int gather_root, double* t_compute_ms,
	double* t_gather_ms);

/* Timing aid for bench.py: runs `iters` executions on device buffers and
 * returns the average duration in milliseconds measured with HIP events on
 * `stream` (the stream the kernels are launched on). */
int avirhip_time_resize(avirhip_plan* plan, const void* src, void* dst,
	int iters, void* stream, double* avg_ms);

/* Synthetic-workload aids for bench.py / smoke (host only): the SURVEY.md
 * 8(c) input generators -- u8: s = seed; per byte s = s*1664525 + 1013904223
 * (uint32), v = s >> 24; f32: the same LCG, x = (s >> 8) * 2^-24 -- and the
 * FNV-1a-64 hash the golden vectors are recorded with (offset basis
 * 1469598103934665603, prime 1099511628211). */
void avirhip_fill_lcg_u8(uint8_t* p, size_t n, uint32_t seed);
void avirhip_fill_lcg_f32(float* p, size_t n, uint32_t seed);
uint64_t avirhip_fnv1a64(const void* p, size_t n);

/* ---------------------------------------------------------------------
 * Front-end mirror: the reference's host-side planner re-implemented inside
 * the library (double precision, -ffp-contract=off, same libm), so that a
 * caller gets "resizeImage" semantics in one call. Names and argument
 * meaning follow avir::CImageResizer (avir.h:4630-4684) and avir::CLancIR
 * (lancir.h:386-390).
 * ------------------------------------------------------------------- */

/* CImageResizerParams (avir.h:2262-2317). */
typedef struct avirhip_params {
	double CorrFltAlpha, CorrFltLen, IntFltAlpha, IntFltCutoff, IntFltLen;
	double LPFltAlpha, LPFltBaseLen, LPFltCutoffMult;
	double HBFltAlpha, HBFltCutoff, HBFltLen;
} avirhip_params;

/* Presets, avir.h:2328-2464. */
typedef enum avirhip_preset {
	AVIRHIP_PARAMS_DEF = 0,
	AVIRHIP_PARAMS_ULR = 1,
	AVIRHIP_PARAMS_LR = 2,
	AVIRHIP_PARAMS_LOW = 3,
	AVIRHIP_PARAMS_HIGH = 4,
	AVIRHIP_PARAMS_ULTRA = 5
} avirhip_preset;

void avirhip_params_preset(int preset, avirhip_params* out);

/* The caller-settable part of CImageResizerVars (avir.h:2516-2547). */
typedef struct avirhip_vars {
	double ox, oy;
	int32_t UseSRGBGamma; /* non-zero: sRGB gamma linearisation (avir.h:2526) */
	int32_t AlphaIndex;
	int32_t BuildMode;    /* -1 = automatic */
	int32_t RndSeed;
} avirhip_vars;

void avirhip_vars_default(avirhip_vars* out);

typedef struct avirhip_resizer avirhip_resizer;

/* CImageResizer(aResBitDepth, aSrcBitDepth, aParams), avir.h:4630-4639.
 * `params` may be NULL (CImageResizerParamsDef). */
int avirhip_resizer_create(int res_bit_depth, int src_bit_depth,
	const avirhip_params* params, avirhip_resizer** out);
void avirhip_resizer_destroy(avirhip_resizer* r);
/* Selects the ditherer class (fpclass::CDitherer, avir.h:4591) of every
 * following resize of this object: AVIRHIP_DITHER_DEF (default) or
 * AVIRHIP_DITHER_ERRD. */
int avirhip_resizer_set_ditherer(avirhip_resizer* r, int dither);
/* Selects the `fptype` packing of the mirrored fpclass (avir.h:4569-4592):
 * 1 = fpclass_def<float> (default), 4 = fpclass_float4 of
 * avir_float4_sse.h (fpclass_def<float4, float>). The arithmetic per channel
 * is the same; what changes is what the reference derives from fppack:
 * ElCount = ceil(ElCountIO / fppack) in the build-mode cost model
 * (avir.h:4786, 6206-6270 -- the automatic BuildMode can differ), the
 * ditherer's rounding and the float-output path (AVIRHIP_DITHER_DEF_RNE),
 * and the CImageResizerVarsBase write-back. The error-diffusion ditherer is
 * only built for fppack 1.
 * AVIRHIP_FPCLASS_DOUBLE = fpclass_def<double> (avir.h:4553-4560): the double
 * pipeline -- tables designed and stored in double, every pass computes in
 * double (the generic kernels; default ditherer only), double output is the
 * vertical pass' in-place result. */
#define AVIRHIP_FPCLASS_DOUBLE 64
int avirhip_resizer_set_fpclass(avirhip_resizer* r, int fppack);

/* Host-only: runs the planner exactly as resizeImage() would for this call
 * and returns the plan description (owned by the library; release with
 * avirhip_plan_desc_free). Needs no GPU. */
int avirhip_resizer_build_desc(avirhip_resizer* r, int src_w, int src_h,
	int src_scanline_size, int new_w, int new_h, int el_count_io, double k,
	const avirhip_vars* vars, int in_type, int out_type,
	avirhip_plan_desc** out);
void avirhip_plan_desc_free(avirhip_plan_desc* desc);

/* The fields of CImageResizerVarsBase (avir.h:2473-2506) as resizeImage()
 * leaves them in the caller's CImageResizerVars (avir.h:4663-4669): the
 * vertical axis is planned last, so k, o, BufLen, BufOffs, ResizeStep and
 * IsResize2 describe its step list. InGammaMult / OutGammaMult are only
 * written when UseSRGBGamma is set (`gamma_valid`). */
typedef struct avirhip_vars_base {
	int32_t ElCount, ElCountIO, fppack, fpalign, elalign, packmode;
	int32_t BufLen[2], BufOffs[2];
	double k, o;
	int32_t ResizeStep, IsResize2;
	int32_t gamma_valid;
	double InGammaMult, OutGammaMult;
} avirhip_vars_base;

/* Host-only (no GPU needed): what resizeImage() with these arguments writes
 * back into *aVars. */
int avirhip_resizer_vars_base(avirhip_resizer* r, int src_w, int src_h,
	int src_scanline_size, int new_w, int new_h, int el_count_io, double k,
	const avirhip_vars* vars, int in_type, int out_type,
	avirhip_vars_base* out);

/* resizeImage<Tin,Tout>(), avir.h:4680-4684. Plans are cached per geometry
 * inside the resizer. Zero-sized source => destination zero-filled
 * (NewWidth*NewHeight elements, avir.h:4686-4692); zero-sized destination
 * => no-op. */
int avirhip_resizer_resize(avirhip_resizer* r, const void* src, int src_mem,
	int src_w, int src_h, int src_scanline_size, void* dst, int dst_mem,
	int new_w, int new_h, int el_count_io, double k,
	const avirhip_vars* vars, int in_type, int out_type, void* stream);

/* Host-only (no GPU needed): avirhip_band_source_rows() for a geometry, from
 * the planner alone -- what a host that deals source rows to the ranks of a
 * sharded frame needs before any device plan exists. */
int avirhip_resizer_band_source_rows(avirhip_resizer* r, int src_w, int src_h,
	int src_scanline_size, int new_w, int new_h, int el_count_io, double k,
	const avirhip_vars* vars, int in_type, int out_type, int row0, int row1,
	int* first, int* last);

/* Returns (and caches) the device plan resizeImage() would use for this
 * geometry; owned by the resizer. */
int avirhip_resizer_get_plan(avirhip_resizer* r, int src_w, int src_h,
	int src_scanline_size, int new_w, int new_h, int el_count_io, double k,
	const avirhip_vars* vars, int in_type, int out_type,
	avirhip_plan** out);

/* CLancIRParams, lancir.h:260-307. */
typedef struct avirhip_lancir_params {
	int32_t SrcSSize, NewSSize;
	double kx, ky, ox, oy, la;
} avirhip_lancir_params;

void avirhip_lancir_params_default(avirhip_lancir_params* out);

typedef struct avirhip_lancir avirhip_lancir;

int avirhip_lancir_create(avirhip_lancir** out);
void avirhip_lancir_destroy(avirhip_lancir* l);

int avirhip_lancir_build_desc(avirhip_lancir* l, int src_w, int src_h,
	int new_w, int new_h, int el_count, const avirhip_lancir_params* params,
	int in_type, int out_type, avirhip_lancir_desc** out);
void avirhip_lancir_desc_free(avirhip_lancir_desc* desc);

/* CLancIR::resizeImage<Tin,Tout>(), lancir.h:386-390. Returns NewHeight on
 * success, 0 on a parameter error (lancir.h:392-407), <0 on a device error. */
int avirhip_lancir_resize(avirhip_lancir* l, const void* src, int src_mem,
	int src_w, int src_h, void* dst, int dst_mem, int new_w, int new_h,
	int el_count, const avirhip_lancir_params* params, int in_type,
	int out_type, void* stream);

/* Host-only: avirhip_band_source_rows() for a CLancIR geometry. */
int avirhip_lancir_band_source_rows(avirhip_lancir* l, int src_w, int src_h,
	int new_w, int new_h, int el_count, const avirhip_lancir_params* params,
	int in_type, int out_type, int row0, int row1, int* first, int* last);

int avirhip_lancir_get_plan(avirhip_lancir* l, int src_w, int src_h,
	int new_w, int new_h, int el_count, const avirhip_lancir_params* params,
	int in_type, int out_type, avirhip_plan** out);

/* Planar calls: n single-channel planes of one geometry -- a channel-first
 * image (C x H x W), a batch (N x C x H x W is N * C planes) -- resized by one
 * call. An extension: the reference has no such call, but it defines what a
 * plane is.
 *   Planes.   The call resizes n_planes >= 1 planes (less: AVIRHIP_EINVAL).
 *             Plane i of the source starts i * src_plane_stride elements behind
 *             `src`, plane i of the result i * dst_plane_stride elements behind
 *             `dst`.
 *   Geometry. Every plane is a src_w x src_h image of ONE channel; its row
 *             pitch is CLancIRParams::SrcSSize / NewSSize elements, or the
 *             width where that is < 1. The planes share one geometry, one
 *             parameter set, one element type per side -- one plan.
 *   Strides.  A plane stride of 0 means tightly packed planes (height x row
 *             pitch). Otherwise it must be at least (height - 1) x pitch +
 *             width, else AVIRHIP_EINVAL. There is no limit of 4 planes.
 *   Result.   Plane i equals, bit for bit, what avir::CLancIR::resizeImage with
 *             ElCount = 1 stores for plane i of the source, for every element
 *             type pair avirhip_lancir_resize takes with one channel. Half and
 *             bfloat16 keep the rule of AVIRHIP_F16 / AVIRHIP_BF16: widened
 *             exactly, the float32 result computed with the plan's gain,
 *             narrowed to nearest even, no clamp.
 *   Rounding. Integer results round by the element's position in its own
 *             scanline of new_w elements: whole groups of four to nearest even
 *             behind the two clamps, the 1-3 element tail by + 0.5 truncation.
 *   Untouched bytes. Nothing outside a result plane's rows is written: not
 *             between rows (NewSSize padding), not between planes, not behind
 *             the last plane.
 *   Parameter errors return what avirhip_lancir_resize returns for them (0:
 *             lancir.h:392-407); src == dst is one of them. A zero-sized source
 *             zero-fills every result plane row by row.
 *   Overlap.  Source and result spans that share bytes: AVIRHIP_EINVAL.
 *   Memory.   Device buffers run asynchronously on `stream`; host buffers are
 *             accepted and staged with plain copies inside the call.
 * uint8, uint16, float32, half and bfloat16 planes on either side, bases that
 * are multiples of the element size, run in ONE launch of a kernel whose lane
 * is one float of one plane (lancp.hip); float64 and uint32 planes, other
 * bases and kernels too long for its tile run the plan's own road once per
 * plane -- the same bits ("Planes").
 *
 * CImageResizer planes. The same call for avir::CImageResizer, with the text
 * above on planes, strides, overlap, memory and untouched bytes unchanged:
 *   Geometry. Every plane is a src_w x src_h image of ONE channel. Source rows
 *             lie SrcScanlineSize elements apart (the width where that is
 *             < 1); result rows are new_w elements, tight: resizeImage has no
 *             destination pitch.
 *   Result.   Plane i equals, bit for bit, what
 *             avir::CImageResizer< fpclass >::resizeImage with ElCountIO = 1
 *             stores for plane i of the source: the same object (ResBitDepth,
 *             SrcBitDepth, parameters, ditherer, fpclass), the same k, the same
 *             aVars. AVIRHIP_F16 / AVIRHIP_BF16 keep their stated rule.
 *             CImageResizerVarsBase is what the ElCountIO = 1 call writes.
 *   Zero sizes. A zero-sized source zero-fills every result plane row by row;
 *             a zero-sized destination is a no-op.
 *   Parameter errors return what avirhip_resizer_resize returns for them.
 * uint8, uint16, float32, half and bfloat16 planes, bases that are multiples of
 * the element size, run in ONE launch of k_avirp (avirp.hip), which interprets
 * the plan's lowered ops of both axes on LDS tiles; float64 planes, sRGB gamma,
 * the error-diffusion ditherer, fpclass_float4 and fpclass_def<double>
 * objects, other bases and filters too long for its tiles run the plan's own
 * road once per plane -- the same bits ("CImageResizer planes").
 *
 * Plane views. `src_mem` / `dst_mem` may be AVIRHIP_MEM_VIEWS, each side on its
 * own: that side's pointer is then a HOST array of n_planes avirhip_plane_view
 * and its plane-stride argument must be 0 (else AVIRHIP_EINVAL). One HWC RGB
 * image is three views { img + c, W * 3, 3 }; a channels-last N x C x H x W
 * batch is N * C views; a list of separately allocated planes is one view
 * each. The array is read inside the call: the caller may overwrite or free
 * it as soon as the call returns, whatever the stream still has to do.
 *   Pitch.    With E = max( elem_stride, 1 ): row_pitch 0 means, for E == 1, the
 *             pitch the call has without views (SrcSSize / NewSSize /
 *             SrcScanlineSize, the width where that is < 1; the tight result
 *             row of CImageResizer), and for E > 1 width * E -- the tight row
 *             of an interleaved image.
 *   Result.   Unchanged: plane i equals, bit for bit, the ElCount = 1 /
 *             ElCountIO = 1 call of the reference on the elements of view i
 *             gathered into a tight plane. CLancIR's integer rounding goes by
 *             the element's position j in its row of new_w elements, not by
 *             its address.
 *   Untouched bytes. Nothing but the new_w x new_h elements of each result
 *             view is written: not the elements between strided neighbours
 *             (the X byte of an RGBX result), not between rows.
 *   Validation, host arithmetic only and before any device call, each
 *             AVIRHIP_EINVAL with a message: a null base; a negative pitch or
 *             stride; where height > 1, row_pitch < ( width - 1 ) * E + 1; a
 *             base that is no multiple of the element size; a view that
 *             leaves the address space.
 *   Overlap.  Source views may overlap each other freely. The byte span of a
 *             result view must not meet the byte span of any source view. Two
 *             result views whose byte spans meet are accepted only as
 *             interleaved planes: the same row_pitch P and elem_stride E,
 *             P % E == 0, bases d elements apart with d % E != 0 -- their
 *             elements are then disjoint. Where height is 1 the pitch
 *             addresses nothing and P is not compared. Any other meeting: AVIRHIP_EINVAL.
 *   Zero-sized source or destination and the front ends' parameter errors
 *             behave as above, view by view.
 *   Memory.   Bases are device pointers; host pixel memory behind a view is
 *             not supported. The other side of such a call, where it has no
 *             views, keeps its plane stride rule and must be device memory at
 *             a base that is a multiple of the element size.
 * Views run in the same ONE launch (k_lancp / k_avirp read each plane's base,
 * pitch and stride from a table the call copies to the device). Where the
 * kernel declines (see above), a view that is not a tight plane at the plan's
 * pitch is gathered into / scattered from a per-call device buffer (allocated
 * and freed in the order of `stream`: no wait for the device), one plane
 * at a time, around the plan's own road; the scatter writes the plane's
 * elements only.
 *
 * Plan level: `plan` is a CLancIR or a CImageResizer plan of one channel; any
 * other channel count returns AVIRHIP_EUNSUPPORTED. Returns AVIRHIP_OK or an
 * error code. */
int avirhip_resize_planes(avirhip_plan* plan, const void* src, int src_mem,
	long long src_plane_stride, void* dst, int dst_mem,
	long long dst_plane_stride, int n_planes, void* stream);

/* Front end: CLancIR::resizeImage over n_planes planes. Returns new_h, 0 on a
 * parameter error, < 0 on any other error. */
int avirhip_lancir_resize_planes(avirhip_lancir* l, const void* src, int src_mem,
	int src_w, int src_h, void* dst, int dst_mem, int new_w, int new_h,
	int n_planes, long long src_plane_stride, long long dst_plane_stride,
	const avirhip_lancir_params* params, int in_type, int out_type, void* stream);

/* Front end: CImageResizer::resizeImage with ElCountIO = 1 over n_planes
 * planes. Returns what avirhip_resizer_resize returns. */
int avirhip_resizer_resize_planes(avirhip_resizer* r, const void* src,
	int src_mem, int src_w, int src_h, int src_scanline_size, void* dst,
	int dst_mem, int new_w, int new_h, int n_planes,
	long long src_plane_stride, long long dst_plane_stride, double k,
	const avirhip_vars* vars, int in_type, int out_type, void* stream);

/* Test hook: the `nth` host allocation (operator new) the CALLING THREAD makes
 * inside the library from now on throws std::bad_alloc (1 = the next one;
 * 0 = off). tests/test_abi.py sweeps it over every allocation of the planning
 * and plan-creation entry points: each must return AVIRHIP_ENOMEM with a
 * message -- never abort the process. Returns the allocations counted on this
 * thread since the previous call. */
long avirhip_debug_fail_alloc(long nth);

/* Test hook: the uint8 sRGB-gamma output stage (applySRGBGamma + default
 * ditherer + unpackScanline, avir.h:2982-3068, 4392-4419, 3155-3215) applied to
 * `npx` float RGBA pixels in device memory, once in the form plans use (the
 * 2 x 256 threshold table, a monotone step function found by bisection on the
 * host) and once as the direct expressions: tests/test_gpu_parity.py sweeps
 * every float bit pattern through both. `tr_mul` >= 1 (1: no bit-depth
 * truncation), `alpha_index` 0..3 or -1. */
int avirhip_debug_gamma_u8(const float* dev_rgba, long npx, double tr_mul,
	int alpha_index, unsigned char* dev_out_table,
	unsigned char* dev_out_direct, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AVIRHIP_H */
