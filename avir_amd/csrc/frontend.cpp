// frontend.cpp -- C ABI of the front-end mirror (include/avirhip.h, second
// half): avirhip_resizer_* mirrors avir::CImageResizer<> (avir.h:4609-5092),
// avirhip_lancir_* mirrors avir::CLancIR (lancir.h:327-755). Each call runs the
// host planner (planner.cpp), caches the uploaded plan per geometry and
// executes it on the device. There is no CPU execution path.

#include "plan.h"
#include "planner.h"
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>

using namespace avirhip;

extern "C" int avirhip_resolve_mem( const void* ptr, int mem );

// Plans cached per geometry (and device), least recently used first out. A
// thumbnailer resizes many geometries through one object: without a bound
// every plan would keep its tables and full-frame scratch until the object
// dies. Bounds: AVIRHIP_CACHE_PLANS plans (default 64) and AVIRHIP_CACHE_BYTES
// of device memory (default 16 GiB). A plan is never dropped while a resize is
// using it, nor after its handle was handed out by *_get_plan().
template< class Key >
struct PlanCache
{
	struct Entry
	{
		avirhip_plan* p;
		unsigned long long tick;
		int busy;    // resizes in flight on the host side
		bool pinned; // handle given to the caller: owned until destruction
	};

	std::map< Key, Entry > m;
	unsigned long long tick = 0;

	Entry* find( const Key& k )
	{
		auto it = m.find( k );

		if( it == m.end() )
		{
			return( nullptr );
		}

		it -> second.tick = ++tick;
		return( &it -> second );
	}

	Entry* insert( const Key& k, avirhip_plan* p )
	{
		Entry e = { p, ++tick, 0, false };
		Entry* r = &( m[ k ] = e );
		trim( r );
		return( r );
	}

	static size_t limit( const char* name, size_t def )
	{
		const char* v = getenv( name );
		return( v != nullptr && atoll( v ) > 0 ? (size_t) atoll( v ) : def );
	}

	void trim( const Entry* keep )
	{
		static const size_t maxn = limit( "AVIRHIP_CACHE_PLANS", 64 );
		static const size_t maxb = limit( "AVIRHIP_CACHE_BYTES",
			(size_t) 16 << 30 );

		while( true )
		{
			size_t bytes = 0;
			auto victim = m.end();

			for( auto it = m.begin(); it != m.end(); ++it )
			{
				bytes += avirhip::plan_device_bytes( it -> second.p );

				if( &it -> second != keep && it -> second.busy == 0 &&
					!it -> second.pinned && ( victim == m.end() ||
					it -> second.tick < victim -> second.tick ))
				{
					victim = it;
				}
			}

			if(( m.size() <= maxn && bytes <= maxb ) || victim == m.end() )
			{
				return;
			}

			// (hipFree inside waits for the plan's queued work)
			avirhip_plan_destroy( victim -> second.p );
			m.erase( victim );
		}
	}

	void clear()
	{
		for( auto& c : m )
		{
			avirhip_plan_destroy( c.second.p );
		}

		m.clear();
	}
};

struct avirhip_resizer
{
	AvirPlanner* planner;
	int dither; // AVIRHIP_DITHER_*: fpclass::CDitherer of the mirrored object
	int fppack; // fpclass::fppack of the mirrored object (1 or 4)
	int f64;    // fpclass_def< double >: the double pipeline
	std::mutex mtx;
	typedef std::tuple< int, int, int, int, int, int, double, double, double,
		int, int, int, int, int, int, int > Key; // ..., ditherer + fppack, device
	PlanCache< Key > cache;
	std::map< Key, avirhip_vars_base > vbcache;
};

struct avirhip_lancir
{
	std::mutex mtx;
	typedef std::tuple< int, int, int, int, int, int, int, double, double,
		double, double, double, int, int, int > Key; // ..., device
	PlanCache< Key > cache;
};

static const avirhip_vars g_defvars = { 0.0, 0.0, 0, -1, -1, 0 };

extern "C" {

void avirhip_fill_lcg_u8( uint8_t* p, size_t n, uint32_t seed )
{
	uint32_t s = seed;

	for( size_t i = 0; i < n; i++ )
	{
		s = s * 1664525u + 1013904223u;
		p[ i ] = (uint8_t) ( s >> 24 );
	}
}

void avirhip_fill_lcg_f32( float* p, size_t n, uint32_t seed )
{
	uint32_t s = seed;

	for( size_t i = 0; i < n; i++ )
	{
		s = s * 1664525u + 1013904223u;
		p[ i ] = (float) ( s >> 8 ) * ( 1.0f / 16777216.0f );
	}
}

uint64_t avirhip_fnv1a64( const void* p, size_t n )
{
	const uint8_t* b = (const uint8_t*) p;
	uint64_t h = 1469598103934665603ULL;

	for( size_t i = 0; i < n; i++ )
	{
		h ^= b[ i ];
		h *= 1099511628211ULL;
	}

	return( h );
}

void avirhip_params_preset( int preset, avirhip_params* p )
{
	if( p == nullptr )
	{
		return;
	}

	// Literals of CImageResizerParams* (avir.h:2300-2464).
	static const double t[ 6 ][ 8 ] = {
		{ 0.97946, 6.4262, 6.41341, 0.7372, 18, 4.76449, 7.55999999999998,
			0.79285 },
		{ 0.95521, 5.70774, 1.00766, 0.74202, 18, 1.6801, 6.62, 0.67821 },
		{ 1, 5.865, 1.79529, 0.74325, 18, 1.87597, 6.89999999999999,
			0.69326 },
		{ 0.99739, 6.20326, 4.6836, 0.73879, 18, 7.86565, 6.91999999999999,
			0.78379 },
		{ 0.97433, 6.87893, 7.74731, 0.73844, 18, 4.8149, 8.07999999999996,
			0.79335 },
		{ 0.99705, 7.42695, 1.71985, 0.7571, 18, 6.71313, 8.27999999999996,
			0.78413 } };

	if( preset < 0 || preset > 5 )
	{
		preset = 0;
	}

	p -> CorrFltAlpha = t[ preset ][ 0 ];
	p -> CorrFltLen = t[ preset ][ 1 ];
	p -> IntFltAlpha = t[ preset ][ 2 ];
	p -> IntFltCutoff = t[ preset ][ 3 ];
	p -> IntFltLen = t[ preset ][ 4 ];
	p -> LPFltAlpha = t[ preset ][ 5 ];
	p -> LPFltBaseLen = t[ preset ][ 6 ];
	p -> LPFltCutoffMult = t[ preset ][ 7 ];
	p -> HBFltAlpha = 1.94609;
	p -> HBFltCutoff = 0.46437;
	p -> HBFltLen = 24;
}

void avirhip_vars_default( avirhip_vars* v )
{
	if( v != nullptr )
	{
		*v = g_defvars;
	}
}

int avirhip_resizer_create( int res_bit_depth, int src_bit_depth,
	const avirhip_params* params, avirhip_resizer** out )
try
{
	avirhip::clear_error();
	if( out == nullptr || res_bit_depth < 1 || res_bit_depth > 16 ||
		src_bit_depth < 0 || src_bit_depth > 16 )
	{
		set_error( "resizer_create: bad arguments" );
		return( AVIRHIP_EINVAL );
	}

	avirhip_params P;

	if( params == nullptr )
	{
		avirhip_params_preset( AVIRHIP_PARAMS_DEF, &P );
	}
	else
	{
		P = *params;
	}

	std::unique_ptr< AvirPlanner > pl( new AvirPlanner( res_bit_depth,
		src_bit_depth, P ));
	avirhip_resizer* r = new avirhip_resizer();
	r -> planner = pl.release();
	r -> dither = AVIRHIP_DITHER_DEF;
	r -> fppack = 1;
	r -> f64 = 0;
	*out = r;
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_resizer_create )

int avirhip_resizer_set_ditherer( avirhip_resizer* r, int dither )
try
{
	avirhip::clear_error();
	if( r == nullptr || ( dither != AVIRHIP_DITHER_DEF &&
		dither != AVIRHIP_DITHER_ERRD ))
	{
		set_error( "set_ditherer: bad arguments" );
		return( AVIRHIP_EINVAL );
	}

	std::lock_guard< std::mutex > lock( r -> mtx );
	r -> dither = dither;
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_resizer_set_ditherer )

int avirhip_resizer_set_fpclass( avirhip_resizer* r, int fppack )
try
{
	avirhip::clear_error();
	if( r == nullptr || ( fppack != 1 && fppack != 4 &&
		fppack != AVIRHIP_FPCLASS_DOUBLE ))
	{
		set_error( "set_fpclass: fppack 1 (float), 4 (float4) or "
			"AVIRHIP_FPCLASS_DOUBLE only" );
		return( AVIRHIP_EINVAL );
	}

	std::lock_guard< std::mutex > lock( r -> mtx );
	r -> f64 = ( fppack == AVIRHIP_FPCLASS_DOUBLE ? 1 : 0 );
	r -> fppack = ( r -> f64 ? 1 : fppack );
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_resizer_set_fpclass )

void avirhip_resizer_destroy( avirhip_resizer* r )
{
	if( r == nullptr )
	{
		return;
	}

	r -> cache.clear();
	delete r -> planner;
	delete r;
}

int avirhip_resizer_build_desc( avirhip_resizer* r, int src_w, int src_h,
	int src_scanline_size, int new_w, int new_h, int el_count_io, double k,
	const avirhip_vars* vars, int in_type, int out_type,
	avirhip_plan_desc** out )
try
{
	avirhip::clear_error();
	if( r == nullptr || out == nullptr )
	{
		set_error( "build_desc: null argument" );
		return( AVIRHIP_EINVAL );
	}

	if( !geometry_ok( "build_desc", src_w, src_h, src_scanline_size, new_w,
		new_h, 0, el_count_io, in_type, out_type ))
	{
		return( AVIRHIP_EINVAL );
	}

	// half / bfloat16 elements are defined by fpclass_def<float>'s float32 call
	// (avirhip.h, AVIRHIP_F16 / AVIRHIP_BF16): fpclass_float4 de-linearises its
	// float results in an output stage of its own, fpclass_def<double> computes
	// other values
	if(( dtype_is_float16_kind( in_type ) ||
		dtype_is_float16_kind( out_type )) && ( r -> fppack == 4 || r -> f64 ))
	{
		set_error( "build_desc: half / bfloat16 elements are built for "
			"fpclass_def<float> only (not %s)", ( r -> f64 ?
			"fpclass_def<double>" : "fpclass_float4" ));
		return( AVIRHIP_EUNSUPPORTED );
	}

	const avirhip_vars& V = ( vars == nullptr ? g_defvars : *vars );
	DescStore* S = r -> planner -> build( src_w, src_h, src_scanline_size,
		new_w, new_h, el_count_io, k, V, in_type, out_type, r -> fppack,
		r -> f64 != 0 );

	if( S == nullptr )
	{
		return( AVIRHIP_EINVAL );
	}

	if(( r -> fppack == 4 || r -> f64 ) && r -> dither != AVIRHIP_DITHER_DEF )
	{
		delete S;
		set_error( "fpclass_float4 / fpclass_def<double>: only the default "
			"ditherer is built" );
		return( AVIRHIP_EUNSUPPORTED );
	}

	S -> d.dither = ( r -> fppack == 4 ? AVIRHIP_DITHER_DEF_RNE :
		r -> dither );
	*out = &S -> d;
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_resizer_build_desc )

void avirhip_plan_desc_free( avirhip_plan_desc* d )
{
	if( d != nullptr )
	{
		delete (DescStore*) ( (char*) d - offsetof( DescStore, d ));
	}
}

int avirhip_resizer_band_source_rows( avirhip_resizer* r, int src_w, int src_h,
	int src_scanline_size, int new_w, int new_h, int el_count_io, double k,
	const avirhip_vars* vars, int in_type, int out_type, int row0, int row1,
	int* first, int* last )
try
{
	avirhip::clear_error();
	if( r == nullptr || first == nullptr || last == nullptr || row0 < 0 ||
		row1 > new_h || row1 <= row0 )
	{
		set_error( "resizer_band_source_rows: bad arguments" );
		return( AVIRHIP_EINVAL );
	}

	avirhip_plan_desc* d = nullptr;
	int rc = avirhip_resizer_build_desc( r, src_w, src_h, src_scanline_size,
		new_w, new_h, el_count_io, k, vars, in_type, out_type, &d );

	if( rc != 0 )
	{
		return( rc );
	}

	struct Free { avirhip_plan_desc* d; ~Free() { avirhip_plan_desc_free( d ); } }
		fr = { d };

	return( desc_band_src_rows( d, row0, row1, first, last ));
}
AVIRHIP_CATCH( avirhip_resizer_band_source_rows )

// Finds or builds the plan of a call. `pin`: the handle leaves the library
// (never evicted); otherwise the entry is marked busy until release().
static int resizer_acquire( avirhip_resizer* r, int src_w, int src_h,
	int src_scanline_size, int new_w, int new_h, int el_count_io, double k,
	const avirhip_vars* vars, int in_type, int out_type, bool pin,
	avirhip_plan** out )
{
	const avirhip_vars& V = ( vars == nullptr ? g_defvars : *vars );

	if( src_scanline_size < 1 )
	{
		src_scanline_size = src_w * el_count_io;
	}

	int dev = 0;
	(void) hipGetDevice( &dev ); // a plan lives on the device it was made on

	std::lock_guard< std::mutex > lock( r -> mtx );
	const avirhip_resizer::Key key( src_w, src_h, src_scanline_size, new_w,
		new_h, el_count_io, k, V.ox, V.oy, V.BuildMode, in_type, out_type,
		( V.UseSRGBGamma ? 1 : 0 ), V.AlphaIndex,
		r -> dither + 16 * r -> fppack + 1024 * r -> f64, dev );

	auto* e = r -> cache.find( key );

	if( e == nullptr )
	{
		avirhip_plan_desc* d = nullptr;
		int rc = avirhip_resizer_build_desc( r, src_w, src_h,
			src_scanline_size, new_w, new_h, el_count_io, k, &V, in_type,
			out_type, &d );

		if( rc != 0 )
		{
			return( rc );
		}

		avirhip_plan* p = nullptr;
		rc = avirhip_plan_create( d, &p );
		avirhip_plan_desc_free( d );

		if( rc != 0 )
		{
			return( rc );
		}

		PlanHold hold( p ); // (the cache's map node may fail to allocate)
		e = r -> cache.insert( key, p );
		hold.release();
	}

	if( pin )
	{
		e -> pinned = true;
	}
	else
	{
		e -> busy++;
	}

	*out = e -> p;
	return( AVIRHIP_OK );
}

static void resizer_release( avirhip_resizer* r, avirhip_plan* p )
{
	std::lock_guard< std::mutex > lock( r -> mtx );

	for( auto& c : r -> cache.m )
	{
		if( c.second.p == p )
		{
			c.second.busy--;
		}
	}

	r -> cache.trim( nullptr ); // scratch may have grown during the call
}

int avirhip_resizer_get_plan( avirhip_resizer* r, int src_w, int src_h,
	int src_scanline_size, int new_w, int new_h, int el_count_io, double k,
	const avirhip_vars* vars, int in_type, int out_type, avirhip_plan** out )
try
{
	avirhip::clear_error();
	if( r == nullptr || out == nullptr )
	{
		set_error( "get_plan: null argument" );
		return( AVIRHIP_EINVAL );
	}

	return( resizer_acquire( r, src_w, src_h, src_scanline_size, new_w, new_h,
		el_count_io, k, vars, in_type, out_type, true, out ));
}
AVIRHIP_CATCH( avirhip_resizer_get_plan )

// CImageResizerVarsBase after resizeImage() (avir.h:2473-2506), from the
// vertical axis of the plan description. The coordinate pair (k, o) walks the
// step list (an upsampling step scales both, a filter step divides them and
// shifts o by its edge pixels); the two flip-flop scanline buffers must hold
// the largest prefix and the largest length + suffix of every step that reads
// or writes them (steps alternate between the buffers, the last one writes
// the destination).
static void fill_vars_base( const avirhip_plan_desc& d, double k0,
	const avirhip_vars& V, avirhip_vars_base* out )
{
	avirhip_vars_base& B = *out;
	memset( &B, 0, sizeof( B ));
	B.ElCount = d.channels; B.ElCountIO = d.channels;
	B.fppack = 1; B.fpalign = 4; B.elalign = 1; B.packmode = 0;

	double k, o = V.oy;

	if( k0 == 0.0 )
	{
		k = (double) d.src_h / d.new_h;
		o += ( k - 1.0 ) * 0.5;
	}
	else
	if( k0 > 0.0 )
	{
		k = k0;
		o += ( k0 - 1.0 ) * 0.5;
	}
	else
	{
		k = -k0;
	}

	int maxpre[ 2 ] = { 0, 0 }, maxlen[ 2 ] = { 0, 0 };
	const int n = d.v.n_steps;

	for( int i = 0; i < n; i++ )
	{
		const avirhip_step& s = d.v.steps[ i ];
		const int ib = i & 1;
		const bool up = ( s.kind == AVIRHIP_STEP_UP_ZEROSTUFF ||
			s.kind == AVIRHIP_STEP_UP_FILTERED );

		if( up )
		{
			k *= s.resample_factor;
			o *= s.resample_factor;
		}
		else
		if( s.kind == AVIRHIP_STEP_FIR )
		{
			k /= s.resample_factor;
			o /= s.resample_factor;
			o += s.edge_pixel_count;
		}
		else
		{
			B.ResizeStep = i;
			B.IsResize2 = ( s.kind == AVIRHIP_STEP_RESIZE2 ? 1 : 0 );
		}

		maxpre[ ib ] = std::max( maxpre[ ib ], s.in_prefix );
		maxlen[ ib ] = std::max( maxlen[ ib ], s.in_len + s.in_suffix );

		if( i + 1 < n )
		{
			const int ob = ib ^ 1;

			if( up )
			{
				maxpre[ ob ] = std::max( maxpre[ ob ], s.out_prefix );
				maxlen[ ob ] = std::max( maxlen[ ob ],
					s.out_len + s.out_suffix );
			}
			else
			{
				maxlen[ ob ] = std::max( maxlen[ ob ], s.out_len );
			}
		}
	}

	for( int i = 0; i < 2; i++ )
	{
		B.BufLen[ i ] = ( maxpre[ i ] + maxlen[ i ]) * d.channels;
		B.BufOffs[ i ] = maxpre[ i ] * d.channels;
	}

	B.k = k; B.o = o;
	B.gamma_valid = ( V.UseSRGBGamma ? 1 : 0 );

	if( V.UseSRGBGamma )
	{
		// avir.h:4744-4763
		B.InGammaMult = ( d.in_type == AVIRHIP_U8 ? 1.0 / 255.0 :
			( d.in_type == AVIRHIP_U16 ? 1.0 / 65535.0 : 1.0 ));

		B.OutGammaMult = ( d.out_type == AVIRHIP_U8 ? 255.0 :
			( d.out_type == AVIRHIP_U16 ? 65535.0 : 1.0 ));
	}
}

int avirhip_resizer_vars_base( avirhip_resizer* r, int src_w, int src_h,
	int src_scanline_size, int new_w, int new_h, int el_count_io, double k,
	const avirhip_vars* vars, int in_type, int out_type,
	avirhip_vars_base* out )
try
{
	avirhip::clear_error();
	if( r == nullptr || out == nullptr )
	{
		set_error( "vars_base: null argument" );
		return( AVIRHIP_EINVAL );
	}

	const avirhip_vars& V = ( vars == nullptr ? g_defvars : *vars );

	if( src_scanline_size < 1 )
	{
		src_scanline_size = src_w * el_count_io;
	}

	const avirhip_resizer::Key key( src_w, src_h, src_scanline_size, new_w,
		new_h, el_count_io, k, V.ox, V.oy, V.BuildMode, in_type, out_type,
		( V.UseSRGBGamma ? 1 : 0 ), V.AlphaIndex,
		16 * r -> fppack + 1024 * r -> f64, 0 );

	{
		std::lock_guard< std::mutex > lock( r -> mtx );
		auto it = r -> vbcache.find( key );

		if( it != r -> vbcache.end() )
		{
			*out = it -> second;
			return( AVIRHIP_OK );
		}
	}

	avirhip_plan_desc* d = nullptr;
	int rc = avirhip_resizer_build_desc( r, src_w, src_h, src_scanline_size,
		new_w, new_h, el_count_io, k, &V, in_type, out_type, &d );

	if( rc != 0 )
	{
		return( rc );
	}

	fill_vars_base( *d, k, V, out );

	if( d -> work_f64 )
	{
		out -> fpalign = 8; // sizeof( double ), avir.h:4578
	}

	if( d -> dither == AVIRHIP_DITHER_DEF_RNE )
	{
		// fpclass_float4: a pixel is one 16-byte fptype (avir.h:4576-4579,
		// 4786-4787); buffer lengths count fptype elements
		const int ch = d -> channels;
		out -> ElCount = ( ch + 3 ) / 4;
		out -> fppack = 4; out -> fpalign = 16;

		for( int i = 0; i < 2; i++ )
		{
			out -> BufLen[ i ] = out -> BufLen[ i ] / ch * out -> ElCount;
			out -> BufOffs[ i ] = out -> BufOffs[ i ] / ch * out -> ElCount;
		}
	}

	avirhip_plan_desc_free( d );

	std::lock_guard< std::mutex > lock( r -> mtx );

	if( r -> vbcache.size() >= 256 )
	{
		r -> vbcache.clear();
	}

	r -> vbcache[ key ] = *out;
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_resizer_vars_base )

int avirhip_resizer_resize( avirhip_resizer* r, const void* src, int src_mem,
	int src_w, int src_h, int src_scanline_size, void* dst, int dst_mem,
	int new_w, int new_h, int el_count_io, double k, const avirhip_vars* vars,
	int in_type, int out_type, void* stream )
try
{
	avirhip::clear_error();
	if( r == nullptr || !avir_dtype_ok( out_type ))
	{
		set_error( "resize: bad arguments" );
		return( AVIRHIP_EINVAL );
	}

	// avir.h:4686-4697: zero-sized source zero-fills NewWidth*NewHeight
	// ELEMENTS (sic, not x channels); zero-sized destination is a no-op.
	if( src_w == 0 || src_h == 0 )
	{
		if( dst == nullptr || new_w < 0 || new_h < 0 )
		{
			set_error( "resize: bad destination" );
			return( AVIRHIP_EINVAL );
		}

		const size_t n = (size_t) new_w * (size_t) new_h *
			dtype_size( out_type );

		dst_mem = avirhip_resolve_mem( dst, dst_mem );

		if( dst_mem == AVIRHIP_MEM_HOST )
		{
			memset( dst, 0, n );
		}
		else
		{
			AVIRHIP_HIPCHECK( hipMemsetAsync( dst, 0, n,
				(hipStream_t) stream ));
		}

		return( AVIRHIP_OK );
	}
	else
	if( new_w == 0 || new_h == 0 )
	{
		return( AVIRHIP_OK );
	}

	avirhip_plan* p = nullptr;
	int rc = resizer_acquire( r, src_w, src_h, src_scanline_size, new_w,
		new_h, el_count_io, k, vars, in_type, out_type, false, &p );

	if( rc != 0 )
	{
		return( rc );
	}

	rc = avirhip_resize( p, src, src_mem, dst, dst_mem, stream );
	resizer_release( r, p );
	return( rc );
}
AVIRHIP_CATCH( avirhip_resizer_resize )

void avirhip_lancir_params_default( avirhip_lancir_params* p )
{
	if( p != nullptr )
	{
		p -> SrcSSize = 0; p -> NewSSize = 0;
		p -> kx = 0.0; p -> ky = 0.0; p -> ox = 0.0; p -> oy = 0.0;
		p -> la = 3.0;
	}
}

int avirhip_lancir_create( avirhip_lancir** out )
try
{
	avirhip::clear_error();
	if( out == nullptr )
	{
		set_error( "lancir_create: null argument" );
		return( AVIRHIP_EINVAL );
	}

	*out = new avirhip_lancir();
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_lancir_create )

void avirhip_lancir_destroy( avirhip_lancir* l )
{
	if( l == nullptr )
	{
		return;
	}

	l -> cache.clear();
	delete l;
}

int avirhip_lancir_build_desc( avirhip_lancir* l, int src_w, int src_h,
	int new_w, int new_h, int el_count, const avirhip_lancir_params* params,
	int in_type, int out_type, avirhip_lancir_desc** out )
try
{
	avirhip::clear_error();
	if( out == nullptr )
	{
		set_error( "lancir_build_desc: null argument" );
		return( AVIRHIP_EINVAL );
	}

	avirhip_lancir_params P;

	if( params == nullptr )
	{
		avirhip_lancir_params_default( &P );
	}
	else
	{
		P = *params;
	}

	if( !geometry_ok( "lancir_build_desc", src_w, src_h, P.SrcSSize, new_w,
		new_h, P.NewSSize, el_count, in_type, out_type ))
	{
		return( AVIRHIP_EINVAL );
	}

	DescStore* S = lancir_build( src_w, src_h, new_w, new_h, el_count, P,
		in_type, out_type );

	if( S == nullptr )
	{
		return( AVIRHIP_EINVAL );
	}

	*out = &S -> ld;
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_lancir_build_desc )

void avirhip_lancir_desc_free( avirhip_lancir_desc* d )
{
	if( d != nullptr )
	{
		delete (DescStore*) ( (char*) d - offsetof( DescStore, ld ));
	}
}

int avirhip_lancir_band_source_rows( avirhip_lancir* l, int src_w, int src_h,
	int new_w, int new_h, int el_count, const avirhip_lancir_params* params,
	int in_type, int out_type, int row0, int row1, int* first, int* last )
try
{
	avirhip::clear_error();
	if( first == nullptr || last == nullptr || row0 < 0 || row1 > new_h ||
		row1 <= row0 )
	{
		set_error( "lancir_band_source_rows: bad arguments" );
		return( AVIRHIP_EINVAL );
	}

	avirhip_lancir_desc* d = nullptr;
	const int rc = avirhip_lancir_build_desc( l, src_w, src_h, new_w, new_h,
		el_count, params, in_type, out_type, &d );

	if( rc != 0 )
	{
		return( rc );
	}

	// the vertical windows in un-padded coordinates, clamped to the image
	// (edge replication of the padding, lancir.h:1541-1594)
	const avirhip_lancir_axis& v = d -> v;
	const int a = v.pos[ row0 ].so - v.padl;
	const int b = v.pos[ row1 - 1 ].so - v.padl + v.kernel_len - 1;
	*first = std::max( 0, std::min( a, src_h - 1 ));
	*last = std::max( 0, std::min( b, src_h - 1 ));
	avirhip_lancir_desc_free( d );
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_lancir_band_source_rows )

static int lancir_acquire( avirhip_lancir* l, int src_w, int src_h,
	int new_w, int new_h, int el_count, const avirhip_lancir_params* params,
	int in_type, int out_type, bool pin, avirhip_plan** out )
{
	avirhip_lancir_params P;

	if( params == nullptr )
	{
		avirhip_lancir_params_default( &P );
	}
	else
	{
		P = *params;
	}

	int dev = 0;
	(void) hipGetDevice( &dev );

	const avirhip_lancir::Key key( src_w, src_h, new_w, new_h, el_count,
		P.SrcSSize, P.NewSSize, P.kx, P.ky, P.ox, P.oy, P.la, in_type,
		out_type, dev );

	std::lock_guard< std::mutex > lock( l -> mtx );
	auto* e = l -> cache.find( key );

	if( e == nullptr )
	{
		avirhip_lancir_desc* d = nullptr;
		int rc = avirhip_lancir_build_desc( l, src_w, src_h, new_w, new_h,
			el_count, &P, in_type, out_type, &d );

		if( rc != 0 )
		{
			return( rc );
		}

		avirhip_plan* p = nullptr;
		rc = avirhip_lancir_plan_create( d, &p );
		avirhip_lancir_desc_free( d );

		if( rc != 0 )
		{
			return( rc );
		}

		PlanHold hold( p );
		e = l -> cache.insert( key, p );
		hold.release();
	}

	if( pin )
	{
		e -> pinned = true;
	}
	else
	{
		e -> busy++;
	}

	*out = e -> p;
	return( AVIRHIP_OK );
}

static void lancir_release( avirhip_lancir* l, avirhip_plan* p )
{
	std::lock_guard< std::mutex > lock( l -> mtx );

	for( auto& c : l -> cache.m )
	{
		if( c.second.p == p )
		{
			c.second.busy--;
		}
	}

	l -> cache.trim( nullptr );
}

int avirhip_lancir_get_plan( avirhip_lancir* l, int src_w, int src_h,
	int new_w, int new_h, int el_count, const avirhip_lancir_params* params,
	int in_type, int out_type, avirhip_plan** out )
try
{
	avirhip::clear_error();
	if( l == nullptr || out == nullptr )
	{
		set_error( "lancir_get_plan: null argument" );
		return( AVIRHIP_EINVAL );
	}

	return( lancir_acquire( l, src_w, src_h, new_w, new_h, el_count, params,
		in_type, out_type, true, out ));
}
AVIRHIP_CATCH( avirhip_lancir_get_plan )

int avirhip_lancir_resize( avirhip_lancir* l, const void* src, int src_mem,
	int src_w, int src_h, void* dst, int dst_mem, int new_w, int new_h,
	int el_count, const avirhip_lancir_params* params, int in_type,
	int out_type, void* stream )
try
{
	avirhip::clear_error();
	// Parameter errors return 0, lancir.h:392-407.
	if( l == nullptr || src_w < 0 || src_h < 0 || new_w <= 0 || new_h <= 0 ||
		src == nullptr || dst == nullptr || src == dst ||
		( params != nullptr && params -> la < 2.0 ))
	{
		return( 0 );
	}

	if( src_w == 0 || src_h == 0 )
	{
		// Zero-filled rows honouring NewSSize, lancir.h:413-425.
		const size_t osl = (size_t) new_w * el_count;
		const size_t nss = ( params != nullptr && params -> NewSSize >= 1 ?
			(size_t) params -> NewSSize : osl );
		const size_t es = dtype_size( out_type );
		dst_mem = avirhip_resolve_mem( dst, dst_mem );

		for( int i = 0; i < new_h; i++ )
		{
			char* op = (char*) dst + (size_t) i * nss * es;

			if( dst_mem == AVIRHIP_MEM_HOST )
			{
				memset( op, 0, osl * es );
			}
			else
			{
				AVIRHIP_HIPCHECK( hipMemsetAsync( op, 0, osl * es,
					(hipStream_t) stream ));
			}
		}

		return( new_h );
	}

	avirhip_plan* p = nullptr;
	int rc = lancir_acquire( l, src_w, src_h, new_w, new_h, el_count, params,
		in_type, out_type, false, &p );

	if( rc != 0 )
	{
		return( rc );
	}

	rc = avirhip_resize( p, src, src_mem, dst, dst_mem, stream );
	lancir_release( l, p );
	return( rc != 0 ? rc : new_h );
}
AVIRHIP_CATCH( avirhip_lancir_resize )

} // extern "C"

// ---------------------------------------------------------------------
// Planar calls (include/avirhip.h, avirhip_resize_planes): n single-channel
// planes of one geometry at a plane stride -- a channel-first image, a batch.
// ---------------------------------------------------------------------

namespace {

// One side of a planar call, in elements: row pitch, plane stride (0 = tightly
// packed), and the bytes from the first plane's first element to the last
// plane's last one.
struct PlanesSide
{
	long pitch, stride;
	size_t es, row_bytes, span_bytes;
};

// Host arithmetic only (no device): the stride rule of the contract.
int planes_side( const char* what, int w, int h, long pitch, long long stride,
	int n_planes, int type, PlanesSide& S )
{
	S.pitch = ( pitch < 1 ? (long) w : pitch );
	S.es = dtype_size( type );
	S.row_bytes = (size_t) w * S.es;
	const long need = (long) ( h - 1 ) * S.pitch + w;

	if( S.pitch < w )
	{
		set_error( "planes: %s row pitch %ld is shorter than a row of %d", what,
			S.pitch, w );
		return( AVIRHIP_EINVAL );
	}

	S.stride = ( stride == 0 ? (long) h * S.pitch : (long) stride );

	if( stride < 0 || S.stride < need )
	{
		set_error( "planes: %s plane stride %lld is shorter than a plane "
			"(%ld elements)", what, stride, need );
		return( AVIRHIP_EINVAL );
	}

	size_t gap = 0;

	if( !mul_fits( (size_t) ( n_planes - 1 ), (size_t) S.stride, S.es, 1, &gap ) ||
		gap + (size_t) need * S.es < gap )
	{
		set_error( "planes: %s planes exceed the address space", what );
		return( AVIRHIP_EINVAL );
	}

	S.span_bytes = gap + (size_t) need * S.es;
	return( AVIRHIP_OK );
}

bool planes_share( const void* a, size_t na, const void* b, size_t nb )
{
	return( (const char*) a < (const char*) b + nb &&
		(const char*) b < (const char*) a + na );
}

// a per-call device allocation (host buffers are staged: not a hot path)
struct DevBuf
{
	void* p;
	DevBuf() : p( nullptr ) {}
	~DevBuf() { if( p != nullptr ) (void) hipFree( p ); }
};

// a per-call device allocation in stream order: freed behind the work that
// was enqueued on `st` before it goes out of scope, without waiting for it
struct StreamBuf
{
	void* p;
	hipStream_t st;
	explicit StreamBuf( hipStream_t s ) : p( nullptr ), st( s ) {}
	~StreamBuf() { if( p != nullptr ) (void) hipFreeAsync( p, st ); }
};

struct CurDevice
{
	int keep;
	bool on;
	explicit CurDevice( int want ) : keep( 0 ), on( false )
	{
		if( hipGetDevice( &keep ) == hipSuccess && keep != want )
		{
			on = ( hipSetDevice( want ) == hipSuccess );
		}
	}
	~CurDevice() { if( on ) (void) hipSetDevice( keep ); }
};

// ---- plane views (include/avirhip.h, "Plane views") ----------------------

// One side of a planar call as it was given: a dense block of planes at a
// plane stride, or (mem == AVIRHIP_MEM_VIEWS) a host array of views.
struct ViewSideArg
{
	const char* what;
	const void* ptr; int mem; long long stride;
	int w, h; long pitch; // the call's own pitch in elements (< 1: the width)
	int type;
};

// One plane of a side, resolved: where it lies, and its byte span [a, b).
struct ViewRec
{
	const char* base; long pb, eb; // row pitch, element stride in bytes
	long long P, E;                // ... in elements
	uintptr_t a, b;
};

// Host arithmetic only: every rule of "Validation" for one side.
int views_side( const ViewSideArg& A, const int n_planes,
	std::vector< ViewRec >& out )
{
	const size_t es = dtype_size( A.type );
	out.resize( (size_t) n_planes );

	if( A.mem != AVIRHIP_MEM_VIEWS )
	{
		PlanesSide S;
		const int rc = planes_side( A.what, A.w, A.h, A.pitch, A.stride,
			n_planes, A.type, S );

		if( rc != 0 )
		{
			return( rc );
		}

		if( (uintptr_t) A.ptr % es != 0 ||
			(uintptr_t) A.ptr + S.span_bytes < (uintptr_t) A.ptr )
		{
			set_error( "planes: beside plane views the %s base must be a "
				"multiple of the element size, its planes within the address "
				"space", A.what );
			return( AVIRHIP_EINVAL );
		}

		const size_t one = ( (size_t) ( A.h - 1 ) * S.pitch + A.w ) * es;

		for( int i = 0; i < n_planes; i++ )
		{
			ViewRec& r = out[ (size_t) i ];
			r.base = (const char*) A.ptr + (size_t) i * S.stride * es;
			r.pb = (long) ( S.pitch * es ); r.eb = (long) es;
			r.P = ( A.h > 1 ? S.pitch : 0 ); r.E = 1;
			r.a = (uintptr_t) r.base; r.b = r.a + one;
		}

		return( AVIRHIP_OK );
	}

	if( A.stride != 0 )
	{
		set_error( "planes: %s plane stride %lld beside plane views (it must "
			"be 0)", A.what, A.stride );
		return( AVIRHIP_EINVAL );
	}

	const avirhip_plane_view* const v = (const avirhip_plane_view*) A.ptr;
	typedef unsigned __int128 u128;
	const u128 lim = (u128) UINTPTR_MAX;

	for( int i = 0; i < n_planes; i++ )
	{
		ViewRec& r = out[ (size_t) i ];

		if( v[ i ].base == nullptr )
		{
			set_error( "planes: %s view %d has a null base", A.what, i );
			return( AVIRHIP_EINVAL );
		}

		if( v[ i ].row_pitch < 0 || v[ i ].elem_stride < 0 )
		{
			set_error( "planes: %s view %d: negative row pitch or element "
				"stride (%lld, %lld)", A.what, i, v[ i ].row_pitch,
				v[ i ].elem_stride );
			return( AVIRHIP_EINVAL );
		}

		if( (uintptr_t) v[ i ].base % es != 0 )
		{
			set_error( "planes: %s view %d: the base is no multiple of the "
				"element size %d", A.what, i, (int) es );
			return( AVIRHIP_EINVAL );
		}

		const u128 E = (u128) std::max( v[ i ].elem_stride, 1LL );
		const u128 row = (u128) ( A.w - 1 ) * E + 1;
		const u128 P = ( v[ i ].row_pitch > 0 ? (u128) v[ i ].row_pitch :
			E > 1 ? (u128) A.w * E :
			(u128) ( A.pitch < 1 ? (long) A.w : A.pitch ));

		if( A.h > 1 && P < row )
		{
			set_error( "planes: %s view %d: row pitch %lld is shorter than a "
				"row (%lld elements)", A.what, i, (long long) P,
				(long long) row );
			return( AVIRHIP_EINVAL );
		}

		// (every factor is below 2^63, the products below 2^127)
		const u128 bytes = ( (u128) ( A.h - 1 ) * P + row ) * es;

		if( E > lim / es || P > lim / es || bytes > lim ||
			(u128) (uintptr_t) v[ i ].base + bytes > lim )
		{
			set_error( "planes: %s view %d exceeds the address space", A.what,
				i );
			return( AVIRHIP_EINVAL );
		}

		r.base = (const char*) v[ i ].base;
		r.pb = (long) ( P * es ); r.eb = (long) ( E * es );
		// (a single row: the pitch addresses nothing and constrains nothing)
		r.P = ( A.h > 1 ? (long long) P : 0 ); r.E = (long long) E;
		r.a = (uintptr_t) r.base; r.b = r.a + (uintptr_t) bytes;
	}

	return( AVIRHIP_OK );
}

// "Overlap": a sort and a sweep on each question. Source spans are merged
// into disjoint intervals and every result span looked up among them. Result
// spans are swept by their starts: those still open at a start all hold that
// byte, so they meet each other and the newcomer -- which must then be an
// interleaved plane of theirs (the same P and E, P % E == 0, a base residue
// mod E that none of them has; at most E spans are open at once).
int views_overlap( const std::vector< ViewRec >& S,
	const std::vector< ViewRec >& D )
{
	std::vector< std::pair< uintptr_t, uintptr_t > > u;

	for( const ViewRec& r : S )
	{
		u.push_back( std::make_pair( r.a, r.b ));
	}

	std::sort( u.begin(), u.end() );
	size_t m = 0;

	for( size_t i = 0; i < u.size(); i++ )
	{
		if( m > 0 && u[ i ].first <= u[ m - 1 ].second )
		{
			u[ m - 1 ].second = std::max( u[ m - 1 ].second, u[ i ].second );
		}
		else
		{
			u[ m++ ] = u[ i ];
		}
	}

	u.resize( m );

	for( const ViewRec& r : D )
	{
		// the first merged interval that ends behind r.a
		size_t lo = 0, hi = u.size();

		while( lo < hi )
		{
			const size_t mid = ( lo + hi ) / 2;

			if( u[ mid ].second > r.a ) hi = mid; else lo = mid + 1;
		}

		if( lo < u.size() && u[ lo ].first < r.b )
		{
			set_error( "planes: source and result planes share bytes" );
			return( AVIRHIP_EINVAL );
		}
	}

	std::vector< const ViewRec* > d;

	for( const ViewRec& r : D )
	{
		d.push_back( &r );
	}

	std::sort( d.begin(), d.end(), []( const ViewRec* x, const ViewRec* y )
		{ return( x -> a < y -> a ); } );

	// the open spans: a heap by end, and their residues
	std::vector< std::pair< uintptr_t, long long > > open; // (end, residue)
	std::vector< long long > res;
	const auto later = []( const std::pair< uintptr_t, long long >& x,
		const std::pair< uintptr_t, long long >& y )
		{ return( x.first > y.first ); };
	long long oP = 0, oE = 0;

	for( const ViewRec* const r : d )
	{
		while( !open.empty() && open.front().first <= r -> a )
		{
			res.erase( std::find( res.begin(), res.end(),
				open.front().second ));
			std::pop_heap( open.begin(), open.end(), later );
			open.pop_back();
		}

		const long long es = r -> eb / r -> E;
		const long long q = (long long) (( r -> a / (uintptr_t) es ) %
			(uintptr_t) r -> E );

		if( !open.empty() )
		{
			if( r -> P != oP || r -> E != oE || r -> P % r -> E != 0 ||
				std::find( res.begin(), res.end(), q ) != res.end() )
			{
				set_error( "planes: result views share bytes and are not "
					"interleaved planes (the same row pitch P and element "
					"stride E, P %% E == 0, bases not a multiple of E apart)" );
				return( AVIRHIP_EINVAL );
			}
		}

		oP = r -> P; oE = r -> E;
		open.push_back( std::make_pair( r -> b, q ));
		std::push_heap( open.begin(), open.end(), later );
		res.push_back( q );
	}

	return( AVIRHIP_OK );
}

// Both sides of a call with plane views on at least one of them: validated,
// and resolved into the kernels' table. `with_src` false: a zero-sized source
// (the result side alone is checked and resolved).
int views_layout( const ViewSideArg& SA, const ViewSideArg& DA,
	const int n_planes, const bool with_src, PlaneViewTable& tab )
{
	std::vector< ViewRec > S, D;

	for( const ViewSideArg* const A : { &SA, &DA })
	{
		if( A -> ptr == nullptr && ( with_src || A == &DA ))
		{
			set_error( "planes: null %s", A -> what );
			return( AVIRHIP_EINVAL );
		}

		if( A -> mem == AVIRHIP_MEM_HOST )
		{
			set_error( "planes: beside plane views the %s must be device "
				"memory", A -> what );
			return( AVIRHIP_EINVAL );
		}
	}

	int rc = views_side( DA, n_planes, D );
	if( rc == 0 && with_src ) rc = views_side( SA, n_planes, S );
	if( rc == 0 ) rc = views_overlap( S, D );

	if( rc != 0 )
	{
		return( rc );
	}

	tab.resize( (size_t) n_planes );

	for( int i = 0; i < n_planes; i++ )
	{
		PlaneViewDev& t = tab[ (size_t) i ];
		t.src = nullptr; t.src_pb = 0; t.src_eb = 0;

		if( with_src )
		{
			t.src = S[ (size_t) i ].base; t.src_pb = S[ (size_t) i ].pb;
			t.src_eb = S[ (size_t) i ].eb;
		}

		t.dst = (char*) D[ (size_t) i ].base; t.dst_pb = D[ (size_t) i ].pb;
		t.dst_eb = D[ (size_t) i ].eb;
	}

	return( AVIRHIP_OK );
}

// A zero-sized source: every result view zero-filled row by row, its
// elements alone.
int views_zero_fill( const PlaneViewTable& tab, const void* dst,
	const int dst_mem, const int w, const int h, const int type,
	hipStream_t st )
{
	const size_t es = dtype_size( type );

	// (validation is behind us: the first call that may reach the device)
	if( dst_mem == AVIRHIP_MEM_AUTO &&
		avirhip_resolve_mem( dst, dst_mem ) == AVIRHIP_MEM_HOST )
	{
		set_error( "planes: beside plane views the result must be device "
			"memory" );
		return( AVIRHIP_EINVAL );
	}

	for( const PlaneViewDev& t : tab )
	{
		if( (size_t) t.dst_eb == es )
		{
			// (one row is its own pitch: a last row may end the allocation)
			AVIRHIP_HIPCHECK( hipMemset2DAsync( t.dst, h > 1 ? (size_t) t.dst_pb :
				(size_t) w * es, 0, (size_t) w * es, h, st ));
			continue;
		}

		for( int y = 0; y < h; y++ )
		{
			// a row as w "rows" of one element at a pitch of the stride
			AVIRHIP_HIPCHECK( hipMemset2DAsync( t.dst + (size_t) y * t.dst_pb,
				w > 1 ? (size_t) t.dst_eb : es, 0, es, w, st ));
		}
	}

	return( AVIRHIP_OK );
}

inline bool has_views( const int src_mem, const int dst_mem )
{
	return( src_mem == AVIRHIP_MEM_VIEWS || dst_mem == AVIRHIP_MEM_VIEWS );
}

// avirhip_resize_planes with plane views on at least one side.
int planes_views_run( avirhip_plan* p, const void* src, int src_mem,
	long long src_plane_stride, void* dst, int dst_mem,
	long long dst_plane_stride, int n_planes, void* stream )
{
	const ViewSideArg SA = { "source", src, src_mem, src_plane_stride,
		p -> src_w, p -> src_h, p -> src_stride, p -> in_type };
	const ViewSideArg DA = { "result", dst, dst_mem, dst_plane_stride,
		p -> new_w, p -> new_h, p -> new_stride, p -> out_type };
	PlaneViewTable tab;
	int rc = views_layout( SA, DA, n_planes, true, tab );

	if( rc != 0 )
	{
		return( rc );
	}

	// (validation is behind us: the first call that may reach the device)
	if(( src_mem == AVIRHIP_MEM_AUTO &&
		avirhip_resolve_mem( src, src_mem ) == AVIRHIP_MEM_HOST ) ||
		( dst_mem == AVIRHIP_MEM_AUTO &&
		avirhip_resolve_mem( dst, dst_mem ) == AVIRHIP_MEM_HOST ))
	{
		set_error( "planes: beside plane views the other side must be device "
			"memory" );
		return( AVIRHIP_EINVAL );
	}

	hipStream_t st = (hipStream_t) stream;
	CurDevice dev( p -> device );
	const char* why = "";
	rc = ( p -> is_lancir ?
		lancp_run( p, nullptr, nullptr, 0, 0, n_planes, st, &why, &tab ) :
		avirp_run( p, nullptr, nullptr, 0, 0, n_planes, st, &why, &tab ));

	if( rc != 1 )
	{
		return( rc );
	}

	// The plan's own road, plane by plane. It reads and writes tight planes at
	// the plan's pitches: a view that is one passes its base; any other is
	// gathered into / scattered from a per-call buffer (one plane a side,
	// used again by the next plane behind it on the stream).
	if( getenv( "AVIRHIP_VERBOSE" ) != nullptr )
	{
		fprintf( stderr, "planes: per-plane road (%s)\n", why );
	}

	const long ses = (long) dtype_size( p -> in_type );
	const long oes = (long) dtype_size( p -> out_type );
	const long spb = (long) p -> src_stride * ses;
	const long dpb = (long) p -> new_stride * oes;
	bool stage_s = false, stage_d = false;

	for( const PlaneViewDev& t : tab )
	{
		stage_s = stage_s || t.src_eb != ses || ( p -> src_h > 1 && t.src_pb != spb );
		stage_d = stage_d || t.dst_eb != oes || ( p -> new_h > 1 && t.dst_pb != dpb );
	}

	// (stream-ordered: allocated and freed behind the work on `st`, so that
	// this road waits for the device no more than the plan's own does)
	StreamBuf bs( st ), bd( st );

	if( stage_s )
	{
		AVIRHIP_HIPCHECK( hipMallocAsync( &bs.p, (size_t) p -> src_h * spb,
			st ));
	}

	if( stage_d )
	{
		AVIRHIP_HIPCHECK( hipMallocAsync( &bd.p, (size_t) p -> new_h * dpb,
			st ));
	}

	rc = AVIRHIP_OK;

	for( int i = 0; i < n_planes && rc == 0; i++ )
	{
		const PlaneViewDev& t = tab[ (size_t) i ];
		const bool gs = ( t.src_eb != ses || ( p -> src_h > 1 && t.src_pb != spb ));
		const bool sd = ( t.dst_eb != oes || ( p -> new_h > 1 && t.dst_pb != dpb ));

		if( gs )
		{
			rc = pview_copy( t.src, t.src_pb, t.src_eb, bs.p, spb, ses,
				p -> src_w, p -> src_h, (int) ses, st );
		}

		if( rc == 0 )
		{
			rc = avirhip_resize( p, gs ? bs.p : (const void*) t.src,
				AVIRHIP_MEM_DEVICE, sd ? bd.p : (void*) t.dst,
				AVIRHIP_MEM_DEVICE, stream );
		}

		if( rc == 0 && sd )
		{
			rc = pview_copy( bd.p, dpb, oes, t.dst, t.dst_pb, t.dst_eb,
				p -> new_w, p -> new_h, (int) oes, st );
		}
	}

	return( rc );
}

} // namespace

extern "C" {

int avirhip_resize_planes( avirhip_plan* p, const void* src, int src_mem,
	long long src_plane_stride, void* dst, int dst_mem,
	long long dst_plane_stride, int n_planes, void* stream )
try
{
	avirhip::clear_error();
	if( p == nullptr || src == nullptr || dst == nullptr )
	{
		set_error( "resize_planes: null argument" );
		return( AVIRHIP_EINVAL );
	}

	if( p -> io_ch != 1 )
	{
		set_error( "resize_planes: a plan of one channel is required (this "
			"one: %s, %d channels)", p -> is_lancir ? "CLancIR" :
			"CImageResizer", p -> io_ch );
		return( AVIRHIP_EUNSUPPORTED );
	}

	if( n_planes < 1 )
	{
		set_error( "resize_planes: n_planes %d", n_planes );
		return( AVIRHIP_EINVAL );
	}

	if( has_views( src_mem, dst_mem ))
	{
		return( planes_views_run( p, src, src_mem, src_plane_stride, dst,
			dst_mem, dst_plane_stride, n_planes, stream ));
	}

	PlanesSide S, D;
	int rc = planes_side( "source", p -> src_w, p -> src_h, p -> src_stride,
		src_plane_stride, n_planes, p -> in_type, S );
	if( rc == 0 ) rc = planes_side( "result", p -> new_w, p -> new_h,
		p -> new_stride, dst_plane_stride, n_planes, p -> out_type, D );

	if( rc != 0 )
	{
		return( rc );
	}

	if( planes_share( src, S.span_bytes, dst, D.span_bytes ))
	{
		set_error( "resize_planes: source and result planes share bytes" );
		return( AVIRHIP_EINVAL );
	}

	src_mem = avirhip_resolve_mem( src, src_mem );
	dst_mem = avirhip_resolve_mem( dst, dst_mem );
	const bool host_src = ( src_mem == AVIRHIP_MEM_HOST );
	const bool host_dst = ( dst_mem == AVIRHIP_MEM_HOST );
	hipStream_t st = (hipStream_t) stream;
	CurDevice dev( p -> device );
	DevBuf bs, bd;
	const char* dsrc = (const char*) src;
	char* ddst = (char*) dst;
	const size_t sps = (size_t) S.stride * S.es, spb = (size_t) S.pitch * S.es;
	const size_t dps = (size_t) D.stride * D.es, dpb = (size_t) D.pitch * D.es;

	// host buffers: staged in the caller's own layout, rows only
	if( host_src )
	{
		AVIRHIP_HIPCHECK( hipMalloc( &bs.p, S.span_bytes ));
		dsrc = (const char*) bs.p;

		for( int i = 0; i < n_planes; i++ )
		{
			AVIRHIP_HIPCHECK( hipMemcpy2DAsync( (char*) bs.p + i * sps, spb,
				(const char*) src + i * sps, spb, S.row_bytes, p -> src_h,
				hipMemcpyHostToDevice, st ));
		}
	}

	if( host_dst )
	{
		AVIRHIP_HIPCHECK( hipMalloc( &bd.p, D.span_bytes ));
		ddst = (char*) bd.p;
	}

	const char* why = "";
	rc = ( p -> is_lancir ?
		lancp_run( p, dsrc, ddst, S.stride, D.stride, n_planes, st, &why ) :
		avirp_run( p, dsrc, ddst, S.stride, D.stride, n_planes, st, &why ));

	if( rc == 1 )
	{
		// the plan's own road, plane by plane (it serialises itself)
		if( getenv( "AVIRHIP_VERBOSE" ) != nullptr )
		{
			fprintf( stderr, "planes: per-plane road (%s)\n", why );
		}

		rc = AVIRHIP_OK;

		for( int i = 0; i < n_planes && rc == 0; i++ )
		{
			rc = avirhip_resize( p, dsrc + i * sps, AVIRHIP_MEM_DEVICE,
				ddst + i * dps, AVIRHIP_MEM_DEVICE, stream );
		}
	}

	if( rc == 0 && host_dst )
	{
		for( int i = 0; i < n_planes; i++ )
		{
			AVIRHIP_HIPCHECK( hipMemcpy2DAsync( (char*) dst + i * dps, dpb,
				ddst + i * dps, dpb, D.row_bytes, p -> new_h,
				hipMemcpyDeviceToHost, st ));
		}
	}

	if( host_src || host_dst )
	{
		AVIRHIP_HIPCHECK( hipStreamSynchronize( st ));
	}

	return( rc );
}
AVIRHIP_CATCH( avirhip_resize_planes )

int avirhip_lancir_resize_planes( avirhip_lancir* l, const void* src,
	int src_mem, int src_w, int src_h, void* dst, int dst_mem, int new_w,
	int new_h, int n_planes, long long src_plane_stride,
	long long dst_plane_stride, const avirhip_lancir_params* params,
	int in_type, int out_type, void* stream )
try
{
	avirhip::clear_error();
	// Parameter errors return 0, as avirhip_lancir_resize (lancir.h:392-407).
	if( l == nullptr || src_w < 0 || src_h < 0 || new_w <= 0 || new_h <= 0 ||
		src == nullptr || dst == nullptr || src == dst ||
		( params != nullptr && params -> la < 2.0 ))
	{
		return( 0 );
	}

	if( n_planes < 1 || in_type < 0 || in_type > AVIRHIP_BF16 || out_type < 0 ||
		out_type > AVIRHIP_BF16 )
	{
		set_error( "lancir_resize_planes: n_planes %d, element types %d, %d",
			n_planes, in_type, out_type );
		return( AVIRHIP_EINVAL );
	}

	// the stride rule and the overlap rule, before any plan exists
	const bool empty = ( src_w == 0 || src_h == 0 );
	if( has_views( src_mem, dst_mem ))
	{
		const ViewSideArg SA = { "source", src, src_mem, src_plane_stride,
			src_w, src_h, params != nullptr ? params -> SrcSSize : 0, in_type };
		const ViewSideArg DA = { "result", dst, dst_mem, dst_plane_stride,
			new_w, new_h, params != nullptr ? params -> NewSSize : 0, out_type };
		PlaneViewTable tab;
		int rc = views_layout( SA, DA, n_planes, !empty, tab );

		if( rc == 0 && empty )
		{
			rc = views_zero_fill( tab, dst, dst_mem, new_w, new_h, out_type,
				(hipStream_t) stream );
			return( rc != 0 ? rc : new_h );
		}

		avirhip_plan* p = nullptr;
		if( rc == 0 ) rc = lancir_acquire( l, src_w, src_h, new_w, new_h, 1,
			params, in_type, out_type, false, &p );

		if( rc != 0 )
		{
			return( rc );
		}

		rc = avirhip_resize_planes( p, src, src_mem, src_plane_stride, dst,
			dst_mem, dst_plane_stride, n_planes, stream );
		lancir_release( l, p );
		return( rc != 0 ? rc : new_h );
	}

	PlanesSide S, D;
	int rc = planes_side( "result", new_w, new_h,
		params != nullptr ? params -> NewSSize : 0, dst_plane_stride, n_planes,
		out_type, D );
	if( rc == 0 && !empty ) rc = planes_side( "source", src_w, src_h,
		params != nullptr ? params -> SrcSSize : 0, src_plane_stride, n_planes,
		in_type, S );

	if( rc != 0 )
	{
		return( rc );
	}

	if( !empty && planes_share( src, S.span_bytes, dst, D.span_bytes ))
	{
		set_error( "lancir_resize_planes: source and result planes share "
			"bytes" );
		return( AVIRHIP_EINVAL );
	}

	if( empty )
	{
		// Zero-filled rows honouring NewSSize, lancir.h:413-425, plane by plane.
		dst_mem = avirhip_resolve_mem( dst, dst_mem );

		for( int i = 0; i < n_planes; i++ )
		{
			char* const op = (char*) dst + (size_t) i * D.stride * D.es;

			if( dst_mem == AVIRHIP_MEM_HOST )
			{
				for( int y = 0; y < new_h; y++ )
				{
					memset( op + (size_t) y * D.pitch * D.es, 0, D.row_bytes );
				}
			}
			else
			{
				AVIRHIP_HIPCHECK( hipMemset2DAsync( op, (size_t) D.pitch * D.es,
					0, D.row_bytes, new_h, (hipStream_t) stream ));
			}
		}

		return( new_h );
	}

	avirhip_plan* p = nullptr;
	rc = lancir_acquire( l, src_w, src_h, new_w, new_h, 1, params, in_type,
		out_type, false, &p );

	if( rc != 0 )
	{
		return( rc );
	}

	rc = avirhip_resize_planes( p, src, src_mem, src_plane_stride, dst,
		dst_mem, dst_plane_stride, n_planes, stream );
	lancir_release( l, p );
	return( rc != 0 ? rc : new_h );
}
AVIRHIP_CATCH( avirhip_lancir_resize_planes )

int avirhip_resizer_resize_planes( avirhip_resizer* r, const void* src,
	int src_mem, int src_w, int src_h, int src_scanline_size, void* dst,
	int dst_mem, int new_w, int new_h, int n_planes,
	long long src_plane_stride, long long dst_plane_stride, double k,
	const avirhip_vars* vars, int in_type, int out_type, void* stream )
try
{
	avirhip::clear_error();
	if( r == nullptr || !avir_dtype_ok( out_type ))
	{
		set_error( "resize_planes: bad arguments" );
		return( AVIRHIP_EINVAL );
	}

	if( n_planes < 1 )
	{
		set_error( "resizer_resize_planes: n_planes %d", n_planes );
		return( AVIRHIP_EINVAL );
	}

	// (a geometry the reference refuses: its error comes from the planner, as
	// avirhip_resizer_resize's does)
	const bool sane = ( src_w >= 0 && src_h >= 0 && new_w >= 0 && new_h >= 0 &&
		avir_dtype_ok( in_type ));
	const bool empty = ( src_w == 0 || src_h == 0 );
	PlanesSide S, D;

	if( sane && ( empty || ( new_w > 0 && new_h > 0 )))
	{
		if( dst == nullptr || ( !empty && src == nullptr ))
		{
			set_error( "resizer_resize_planes: null image" );
			return( AVIRHIP_EINVAL );
		}

		if( has_views( src_mem, dst_mem ))
		{
			if( new_w == 0 || new_h == 0 )
			{
				return( AVIRHIP_OK );
			}

			const ViewSideArg SA = { "source", src, src_mem, src_plane_stride,
				src_w, src_h, src_scanline_size, in_type };
			const ViewSideArg DA = { "result", dst, dst_mem, dst_plane_stride,
				new_w, new_h, 0, out_type };
			PlaneViewTable tab;
			int rc = views_layout( SA, DA, n_planes, !empty, tab );

			if( rc == 0 && empty )
			{
				return( views_zero_fill( tab, dst, dst_mem, new_w, new_h,
					out_type, (hipStream_t) stream ));
			}

			avirhip_plan* p = nullptr;
			if( rc == 0 ) rc = resizer_acquire( r, src_w, src_h,
				src_scanline_size, new_w, new_h, 1, k, vars, in_type, out_type,
				false, &p );

			if( rc != 0 )
			{
				return( rc );
			}

			rc = avirhip_resize_planes( p, src, src_mem, src_plane_stride,
				dst, dst_mem, dst_plane_stride, n_planes, stream );
			resizer_release( r, p );
			return( rc );
		}

		// the stride rule and the overlap rule, before any plan exists
		int rc = ( new_w > 0 && new_h > 0 ? planes_side( "result", new_w, new_h,
			0, dst_plane_stride, n_planes, out_type, D ) : AVIRHIP_OK );
		if( rc == 0 && !empty ) rc = planes_side( "source", src_w, src_h,
			src_scanline_size, src_plane_stride, n_planes, in_type, S );

		if( rc != 0 )
		{
			return( rc );
		}

		if( !empty && planes_share( src, S.span_bytes, dst, D.span_bytes ))
		{
			set_error( "resizer_resize_planes: source and result planes share "
				"bytes" );
			return( AVIRHIP_EINVAL );
		}
	}

	if( sane && empty )
	{
		// avir.h:4686-4697, plane by plane: rows of new_w elements, tight
		if( new_w == 0 || new_h == 0 )
		{
			return( AVIRHIP_OK );
		}

		dst_mem = avirhip_resolve_mem( dst, dst_mem );

		for( int i = 0; i < n_planes; i++ )
		{
			char* const op = (char*) dst + (size_t) i * D.stride * D.es;

			if( dst_mem == AVIRHIP_MEM_HOST )
			{
				for( int y = 0; y < new_h; y++ )
				{
					memset( op + (size_t) y * D.pitch * D.es, 0, D.row_bytes );
				}
			}
			else
			{
				AVIRHIP_HIPCHECK( hipMemset2DAsync( op, (size_t) D.pitch * D.es,
					0, D.row_bytes, new_h, (hipStream_t) stream ));
			}
		}

		return( AVIRHIP_OK );
	}
	else
	if( sane && ( new_w == 0 || new_h == 0 ))
	{
		return( AVIRHIP_OK );
	}

	avirhip_plan* p = nullptr;
	int rc = resizer_acquire( r, src_w, src_h, src_scanline_size, new_w,
		new_h, 1, k, vars, in_type, out_type, false, &p );

	if( rc != 0 )
	{
		return( rc );
	}

	if( !sane )
	{
		resizer_release( r, p );
		set_error( "resizer_resize_planes: bad geometry" );
		return( AVIRHIP_EINVAL );
	}

	rc = avirhip_resize_planes( p, src, src_mem, src_plane_stride, dst,
		dst_mem, dst_plane_stride, n_planes, stream );
	resizer_release( r, p );
	return( rc );
}
AVIRHIP_CATCH( avirhip_resizer_resize_planes )

} // extern "C"
