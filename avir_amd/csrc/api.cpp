// api.cpp -- the C ABI of libavirhip (include/avirhip.h): plan validation and
// lowering, device upload, scratch management and pass orchestration. The
// arithmetic lives in generic.hip / fused.hip; the host-side planner mirror
// (avirhip_resizer_*, avirhip_lancir_*) lives in planner.cpp.

#include "plan.h"
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <atomic>
#include <thread>
#include <system_error>
#include <new>
#include <stdexcept>

namespace avirhip {

static thread_local char g_err[ 512 ] = "";

void set_error( const char* fmt, ... )
{
	va_list ap;
	va_start( ap, fmt );
	vsnprintf( g_err, sizeof( g_err ), fmt, ap );
	va_end( ap );
}

// (every extern "C" entry point begins with this: the message belongs to the
// calling thread's most recent call, never to an older failure)
void clear_error()
{
	g_err[ 0 ] = 0;
}

size_t dtype_size( int t )
{
	return( t == AVIRHIP_U8 ? 1 : t == AVIRHIP_U16 ? 2 : t == AVIRHIP_F32 ? 4 :
		t == AVIRHIP_U32 ? 4 : dtype_is_float16_kind( t ) ? 2 : 8 );
}

int guard_fail( const char* fn ) noexcept
{
	// (called from a catch( ... ) handler: rethrow to see what is in flight)
	try
	{
		throw;
	}
	catch( const std::bad_alloc& )
	{
		set_error( "%s: out of host memory", fn );
		return( AVIRHIP_ENOMEM );
	}
	catch( const std::length_error& e )
	{
		// (a container asked for more than max_size(): the same condition)
		set_error( "%s: out of host memory (%s)", fn, e.what() );
		return( AVIRHIP_ENOMEM );
	}
	catch( const std::exception& e )
	{
		set_error( "%s: internal error: %s", fn, e.what() );
	}
	catch( ... )
	{
		set_error( "%s: internal error (unknown exception)", fn );
	}

	return( AVIRHIP_EINTERNAL );
}

bool mul_fits( size_t a, size_t b, size_t c, size_t d, size_t* out )
{
	size_t r = 0;

	if( __builtin_mul_overflow( a, b, &r ) || __builtin_mul_overflow( r, c, &r ) ||
		__builtin_mul_overflow( r, d, &r ))
	{
		return( false );
	}

	if( out != nullptr )
	{
		*out = r;
	}

	return( true );
}

bool geometry_ok( const char* fn, int src_w, int src_h, long src_stride,
	int new_w, int new_h, long new_stride, int ch, int in_type, int out_type )
{
	if( src_w < 0 || src_h < 0 || new_w < 0 || new_h < 0 || ch < 1 || ch > 4 )
	{
		set_error( "%s: bad image geometry", fn );
		return( false );
	}

	const long INTMAX = 0x7fffffffL;
	const long se = (long) src_w * ch, ne = (long) new_w * ch;

	if( src_stride < 1 ) src_stride = se;
	if( new_stride < 1 ) new_stride = ne;

	// a float copy of either image (16 bytes per RGBA pixel) is the largest
	// buffer a plan may allocate per pixel
	if( se > INTMAX || ne > INTMAX || src_stride > INTMAX || new_stride > INTMAX ||
		!mul_fits( (size_t) src_stride, (size_t) src_h, 16, 1 ) ||
		!mul_fits( (size_t) new_stride, (size_t) new_h, 16, 1 ) ||
		!mul_fits( (size_t) src_w, (size_t) new_h, 16 * ch, 1 ) ||
		!mul_fits( (size_t) new_w, (size_t) src_h, 16 * ch, 1 ) ||
		dtype_size( in_type ) == 0 || dtype_size( out_type ) == 0 )
	{
		set_error( "%s: image of %d x %d x %d -> %d x %d elements does not fit "
			"int rows / size_t bytes", fn, src_w, src_h, ch, new_w, new_h );
		return( false );
	}

	return( true );
}

PlanHold :: ~PlanHold()
{
	if( p != nullptr )
	{
		avirhip_plan_destroy( p );
	}
}

template< typename T >
static int upload( avirhip_plan* p, const std::vector< T >& h, T** d )
{
	*d = nullptr;

	if( h.empty() )
	{
		return( AVIRHIP_OK );
	}

	void* q = nullptr;
	AVIRHIP_HIPCHECK( hipMalloc( &q, h.size() * sizeof( T )));
	p -> allocs.push_back( q );
	p -> alloc_bytes += h.size() * sizeof( T );
	AVIRHIP_HIPCHECK( hipMemcpy( q, h.data(), h.size() * sizeof( T ),
		hipMemcpyHostToDevice ));

	*d = (T*) q;
	return( AVIRHIP_OK );
}

static int dev_alloc( avirhip_plan* p, size_t bytes, void** out )
{
	void* q = nullptr;
	AVIRHIP_HIPCHECK( hipMalloc( &q, bytes ));
	p -> allocs.push_back( q );
	p -> alloc_bytes += bytes;
	*out = q;
	return( AVIRHIP_OK );
}

// a scratch buffer of at least `need` bytes (a larger one replaces it)
static int grow( avirhip_plan* p, void** buf, size_t* have, size_t need )
{
	if( *have < need )
	{
		void* q;
		const int rc = dev_alloc( p, need, &q );
		if( rc != 0 ) return( rc );
		*buf = q;
		*have = need;
	}

	return( AVIRHIP_OK );
}

// a scratch buffer of `n` floats, allocated when it is first needed
static int need_floats( avirhip_plan* p, float** buf, size_t n )
{
	if( *buf == nullptr )
	{
		void* q;
		const int rc = dev_alloc( p, n * sizeof( float ), &q );
		if( rc != 0 ) return( rc );
		*buf = (float*) q;
	}

	return( AVIRHIP_OK );
}

// ---- lowering of one AVIR axis (see plan.h for the view semantics) ----

// a step's tables in the working type F: the float or the double fields of
// the public structures (include/avirhip.h); `x` of an avirhip_rpos
template< typename F >
struct StepTab
{
	const F* flt; const F* suffix_dc; const F* prefix_dc; const F* phase_taps;
	F avirhip_rpos::* x;
};

template< typename F >
static StepTab< F > step_tab( const avirhip_step& s )
{
	if constexpr( sizeof( F ) == sizeof( double ))
	{
		return( StepTab< F >{ s.flt64, s.suffix_dc64, s.prefix_dc64,
			s.phase_taps64, &avirhip_rpos::x64 });
	}
	else
	{
		return( StepTab< F >{ s.flt, s.suffix_dc, s.prefix_dc, s.phase_taps,
			&avirhip_rpos::x });
	}
}

template< typename T >
static void null_tabs( const T& t )
{
	t.d_flt = nullptr; t.d_coef = nullptr; t.d_sdc = nullptr; t.d_pdc = nullptr;
}

// (F: float, or double for a double plan; the other type's tables stay empty)
template< typename F >
static int lower_axis_as( const avirhip_axis& ax, int src_len, int dst_len,
	LAxis& L )
{
	L.ops.clear();
	L.src_len = src_len;
	L.dst_len = dst_len;

	if( ax.n_steps < 1 || ax.steps == nullptr )
	{
		set_error( "axis has no steps" );
		return( AVIRHIP_EINVAL );
	}

	int cur_len = src_len;
	bool zs = false;      // a zero-stuff view is pending for the next step
	int zs_in_len = 0, zs_mmax = 0, zs_prefix = 0;
	bool prev_upf = false;
	int prev_prefix = 0, prev_total = 0;

	for( int si = 0; si < ax.n_steps; si++ )
	{
		const avirhip_step& s = ax.steps[ si ];
		const StepTab< F > st = step_tab< F >( s );

		if( s.in_len != cur_len )
		{
			set_error( "step %d: in_len %d != previous out_len %d", si,
				s.in_len, cur_len );
			return( AVIRHIP_EINVAL );
		}

		if( zs && s.kind != AVIRHIP_STEP_RESIZE2 )
		{
			set_error( "step %d: zero-stuff upsample must be followed by "
				"RESIZE2", si );
			return( AVIRHIP_EUNSUPPORTED );
		}

		LOp op;
		const auto ot = op_tab< F >( op );
		op.type = 0; op.view = ( prev_upf ? VIEW_RAW : VIEW_CLAMP );
		op.in_len = s.in_len; op.in_prefix = ( prev_upf ? prev_prefix : 0 );
		op.zs_mmax = 0x7fffffff;
		op.out_len = s.out_len; op.out_prefix = 0; op.out_total = s.out_len;
		op.rf = 1; op.lat = 0; op.e = 0;
		op.maxtaps = 0; op.d_start = nullptr; op.d_ntaps = nullptr;
		op.flen = 0; op.up_inprefix = 0; op.up_R = 0; op.sdc_len = 0;
		op.pdc_len = 0; op.pdc_d0 = 0;
		null_tabs( op_tab< float >( op ));
		null_tabs( op_tab< double >( op ));

		if( s.kind == AVIRHIP_STEP_FIR )
		{
			if( s.resample_factor < 1 || st.flt == nullptr ||
				s.flt_latency < 0 || s.flt_len != 2 * s.flt_latency + 1 )
			{
				set_error( "step %d: malformed FIR (len %d, latency %d)", si,
					s.flt_len, s.flt_latency );
				return( AVIRHIP_EINVAL );
			}

			op.type = OP_FIR;
			op.rf = s.resample_factor;
			op.lat = s.flt_latency;
			op.e = s.edge_pixel_count;

			ot.h_flt.assign( st.flt + s.flt_latency, st.flt + s.flt_len );

			if( prev_upf )
			{
				// reads in[rf*(n-e) +- lat] of the raw upsample buffer
				const int lo = -op.e * op.rf - op.lat + prev_prefix;
				const int hi = op.rf * ( s.out_len - 1 - op.e ) + op.lat +
					prev_prefix;

				if( lo < 0 || hi >= prev_total )
				{
					set_error( "step %d: FIR reads outside upsample buffer",
						si );
					return( AVIRHIP_EINVAL );
				}
			}

			L.ops.push_back( op );
			prev_upf = false;
		}
		else
		if( s.kind == AVIRHIP_STEP_UP_ZEROSTUFF )
		{
			if( s.resample_factor != 2 || prev_upf )
			{
				set_error( "step %d: zero-stuff upsample supports factor 2 "
					"only", si );
				return( AVIRHIP_EUNSUPPORTED );
			}

			zs = true;
			zs_in_len = s.in_len;
			zs_mmax = s.in_len - 1 + s.out_suffix / 2;
			zs_prefix = s.out_prefix;
		}
		else
		if( s.kind == AVIRHIP_STEP_UP_FILTERED )
		{
			if( s.resample_factor < 2 || st.flt == nullptr ||
				s.flt_len < 1 || prev_upf )
			{
				set_error( "step %d: malformed filtered upsample", si );
				return( AVIRHIP_EINVAL );
			}

			op.type = OP_UPF;
			op.view = VIEW_CLAMP;
			op.rf = s.resample_factor;
			op.flen = s.flt_len;

			ot.h_flt.assign( st.flt, st.flt + s.flt_len );

			op.up_inprefix = s.in_prefix;
			op.up_R = s.in_prefix + s.in_len + s.in_suffix;
			op.sdc_len = s.suffix_dc_len;
			op.pdc_len = s.prefix_dc_len;
			op.pdc_d0 = s.out_prefix - s.in_prefix * s.resample_factor;
			op.out_prefix = s.out_prefix;
			op.out_total = s.out_prefix + s.out_len + s.out_suffix;

			if( op.pdc_d0 < 0 ||
				op.pdc_d0 + op.pdc_len > op.out_total ||
				op.up_R * op.rf + op.sdc_len > op.out_total ||
				( op.up_R - 1 ) * op.rf + op.flen > op.out_total )
			{
				set_error( "step %d: upsample tails exceed buffer", si );
				return( AVIRHIP_EINVAL );
			}

			// stash DC tails behind the filter taps: [flt | sdc | pdc]
			if( s.suffix_dc_len > 0 )
				ot.h_flt.insert( ot.h_flt.end(), st.suffix_dc,
					st.suffix_dc + s.suffix_dc_len );
			if( s.prefix_dc_len > 0 )
				ot.h_flt.insert( ot.h_flt.end(), st.prefix_dc,
					st.prefix_dc + s.prefix_dc_len );

			L.ops.push_back( op );
			prev_upf = true;
			prev_prefix = op.out_prefix;
			prev_total = op.out_total;
		}
		else
		if( s.kind == AVIRHIP_STEP_RESIZE || s.kind == AVIRHIP_STEP_RESIZE2 )
		{
			const bool r2 = ( s.kind == AVIRHIP_STEP_RESIZE2 );

			if( r2 != zs )
			{
				set_error( "step %d: RESIZE2 needs a preceding zero-stuff "
					"upsample (and RESIZE must not have one)", si );
				return( AVIRHIP_EUNSUPPORTED );
			}

			if( s.rpos == nullptr || st.phase_taps == nullptr ||
				s.bank_filter_len < 2 || s.n_phases < 1 ||
				( s.bank_order != 0 && s.bank_order != 1 ))
			{
				set_error( "step %d: malformed resize step", si );
				return( AVIRHIP_EINVAL );
			}

			const int fl = s.bank_filter_len;
			const int fsz = fl * ( s.bank_order + 1 );
			op.type = OP_GATHER;
			op.maxtaps = ( r2 ? ( fl + 1 ) / 2 : fl );
			op.h_start.resize( s.out_len );
			op.h_ntaps.resize( s.out_len );

			ot.h_coef.assign( (size_t) s.out_len * op.maxtaps, (F) 0.0 );

			if( r2 )
			{
				op.view = VIEW_ZS;
				op.in_len = zs_in_len;
				op.zs_mmax = zs_mmax;
			}

			for( int j = 0; j < s.out_len; j++ )
			{
				const avirhip_rpos& rp = s.rpos[ j ];

				if( rp.phase < 0 || rp.phase >= s.n_phases || rp.ftp_off < 0 ||
					rp.fl < 1 || rp.ftp_off + rp.fl > fl )
				{
					set_error( "step %d: bad rpos[%d]", si, j );
					return( AVIRHIP_EINVAL );
				}

				const int stp = ( r2 ? 2 : 1 );
				int nt = 0;

				const F* ftp = st.phase_taps + (size_t) rp.phase * fsz +
					rp.ftp_off;
				const F* ftp2 = ftp + fl;
				F* cf = &ot.h_coef[ (size_t) j * op.maxtaps ];

				for( int i = 0; i < rp.fl; i += stp )
				{
					// xx = ftp[i] + ftp2[i]*x in F (avir.h:3945, 4177);
					// this TU is compiled -ffp-contract=off.
					if( s.bank_order == 1 )
					{
						const F t = ftp2[ i ] * rp.*st.x;
						cf[ nt ] = ftp[ i ] + t;
					}
					else
					{
						cf[ nt ] = ftp[ i ];
					}

					nt++;
				}

				op.h_ntaps[ j ] = nt;
				int lo, hi;

				if( r2 )
				{
					if( rp.src_offs_px & 1 )
					{
						set_error( "step %d: odd RESIZE2 offset at %d", si,
							j );
						return( AVIRHIP_EINVAL );
					}

					op.h_start[ j ] = rp.src_offs_px / 2;
					lo = op.h_start[ j ];
					hi = lo + nt - 1;

					if( 2 * lo < -zs_prefix )
					{
						set_error( "step %d: RESIZE2 reads before the "
							"upsample buffer at %d", si, j );
						return( AVIRHIP_EINVAL );
					}
				}
				else
				{
					op.h_start[ j ] = rp.src_offs_px;
					lo = rp.src_offs_px;
					hi = lo + nt - 1;

					if( prev_upf &&
						( lo + prev_prefix < 0 || hi + prev_prefix >= prev_total ))
					{
						set_error( "step %d: RESIZE reads outside the "
							"upsample buffer at %d", si, j );
						return( AVIRHIP_EINVAL );
					}
				}
			}

			L.ops.push_back( op );
			prev_upf = false;
			zs = false;
		}
		else
		{
			set_error( "step %d: unknown kind %d", si, s.kind );
			return( AVIRHIP_EINVAL );
		}

		cur_len = s.out_len;
	}

	if( zs || prev_upf || L.ops.empty() || cur_len != dst_len )
	{
		set_error( "axis does not end in a filtering/resizing step of length "
			"%d (got %d)", dst_len, cur_len );
		return( AVIRHIP_EINVAL );
	}

	return( AVIRHIP_OK );
}

static int lower_axis( const avirhip_axis& ax, int src_len, int dst_len,
	LAxis& L, const bool f64 = false )
{
	return( f64 ? lower_axis_as< double >( ax, src_len, dst_len, L ) :
		lower_axis_as< float >( ax, src_len, dst_len, L ));
}

// an op's filter taps of type F, with the DC tails stashed behind them
template< typename F >
static int upload_flt( avirhip_plan* p, LOp& op )
{
	const auto t = op_tab< F >( op );
	const int rc = upload( p, t.h_flt, &t.d_flt );

	if( rc == 0 && op.type == OP_UPF )
	{
		t.d_sdc = t.d_flt + op.flen;
		t.d_pdc = t.d_sdc + op.sdc_len;
	}

	return( rc );
}

static int upload_axis( avirhip_plan* p, LAxis& L )
{
	for( size_t i = 0; i < L.ops.size(); i++ )
	{
		LOp& op = L.ops[ i ];
		const auto tf = op_tab< float >( op );
		const auto td = op_tab< double >( op );
		int rc;

		if(( rc = upload_flt< float >( p, op )) != 0 ) return( rc );
		if(( rc = upload( p, op.h_start, &op.d_start )) != 0 ) return( rc );
		if(( rc = upload( p, op.h_ntaps, &op.d_ntaps )) != 0 ) return( rc );
		if(( rc = upload( p, tf.h_coef, &tf.d_coef )) != 0 ) return( rc );
		if(( rc = upload_flt< double >( p, op )) != 0 ) return( rc );
		if(( rc = upload( p, td.h_coef, &td.d_coef )) != 0 ) return( rc );
	}

	return( AVIRHIP_OK );
}

// Needed logical input range of `op` for logical outputs [a, b].
void need_range( const LOp& op, int a, int b, int& ia, int& ib )
{
	if( op.type == OP_FIR )
	{
		ia = op.rf * ( a - op.e ) - op.lat;
		ib = op.rf * ( b - op.e ) + op.lat;
	}
	else
	if( op.type == OP_GATHER )
	{
		ia = 0x7fffffff;
		ib = -0x7fffffff;

		for( int j = a; j <= b; j++ )
		{
			ia = std::min( ia, op.h_start[ j ]);
			ib = std::max( ib, op.h_start[ j ] + op.h_ntaps[ j ] - 1 );
		}
	}
	else
	{
		ia = 0;
		ib = op.in_len - 1;
		return;
	}

	if( op.view == VIEW_RAW )
	{
		return; // logical indices of the upsample buffer (may be negative)
	}

	ia = std::max( 0, std::min( ia, op.in_len - 1 ));
	ib = std::max( 0, std::min( ib, op.in_len - 1 ));
}

// An AVIR plan's kernels read float pixels of the plan's channel count, without
// gamma: any other source goes through the pack pass's copy (`packed`)
static bool avir_need_pack( const avirhip_plan* p )
{
	return( p -> gamma || p -> in_type != AVIRHIP_F32 || p -> ch != p -> io_ch );
}

// float output is the vertical pass' in-place result (avir.h:4956-4979):
// with gamma it stays linear, only the other output types are
// de-linearised in the epilogue
// (fpclass_float4 has no in-place output: its float results pass through
// the output stage like every other type, which matters with gamma)
static bool avir_direct( const avirhip_plan* p )
{
	return( p -> out_type == AVIRHIP_F32 && p -> ch == p -> io_ch &&
		!( p -> fp4 && p -> gamma ));
}

// The float copies a call may need, allocated up front: every road but
// k_dnfh's and the pass kernels' with half / bfloat16 pixels on a side
// (avir_road: `lazy`) calls this first. Those skip it, and road_pack (`packed`)
// and road_need_res (`resbuf`) allocate each when something is about to use it
// -- the same sizes as here, so after this function they are no-ops.
static int ensure_scratch( avirhip_plan* p )
{
	int rc;

	if( p -> is_lancir )
	{
		if(( rc = need_floats( p, &p -> resbuf, (size_t) p -> new_h *
			p -> src_w * p -> ch )) != 0 ) return( rc );

		if( !( p -> out_type == AVIRHIP_F32 && p -> l_unity ) &&
			( rc = need_floats( p, &p -> lres, (size_t) p -> new_h *
			p -> new_w * p -> ch )) != 0 ) return( rc );

		return( AVIRHIP_OK );
	}

	if( avir_need_pack( p ) &&
		( rc = need_floats( p, &p -> packed, (size_t) p -> src_w * p -> src_h *
		p -> ch )) != 0 ) return( rc );

	if( !avir_direct( p ) &&
		( rc = need_floats( p, &p -> resbuf, (size_t) p -> new_w * p -> new_h *
		p -> ch )) != 0 ) return( rc );

	return( AVIRHIP_OK );
}

template< typename F >
int ensure_generic_scratch( avirhip_plan* p )
{
	const PlanBufs< F > B = plan_bufs< F >( p );
	int rc;
	void* q;

	if( B.hbuf.empty() )
	{
		for( size_t i = 0; i < p -> h.ops.size(); i++ )
		{
			if(( rc = dev_alloc( p, (size_t) p -> h.ops[ i ].out_total *
				p -> src_h * p -> ch * sizeof( F ), &q )) != 0 )
				return( rc );
			B.hbuf.push_back( (F*) q );
		}

		for( size_t i = 0; i + 1 < p -> v.ops.size(); i++ )
		{
			if(( rc = dev_alloc( p, (size_t) p -> v.ops[ i ].out_total *
				p -> new_w * p -> ch * sizeof( F ), &q )) != 0 )
				return( rc );
			B.vbuf.push_back( (F*) q );
		}
	}

	return( AVIRHIP_OK );
}

// Backward range propagation through the vertical chain.
VRanges v_ranges( const LAxis& v, int row0, int row1 )
{
	const int nv = (int) v.ops.size();
	VRanges R;
	R.va.resize( nv ); R.vb.resize( nv );
	int a = row0, b = row1 - 1;

	for( int i = nv - 1; i >= 0; i-- )
	{
		const LOp& op = v.ops[ i ];
		R.va[ i ] = a;
		R.vb[ i ] = b;

		if( op.type == OP_UPF )
		{
			R.va[ i ] = -op.out_prefix;
			R.vb[ i ] = op.out_total - op.out_prefix - 1;
		}

		int ia, ib;
		need_range( op, R.va[ i ], R.vb[ i ], ia, ib );
		a = ia;
		b = ib;
	}

	R.ya = a; R.yb = b; // FltBuf rows needed
	return( R );
}

// Runs the generic chain for output rows [row0, row1) into `dst` (a surface
// of F whose row `row0` is at dst).
template< typename F >
int run_generic( avirhip_plan* p, const F* src, long src_stride, F* dst,
	int row0, int row1, hipStream_t st )
{
	int rc = ensure_generic_scratch< F >( p );
	if( rc != 0 ) return( rc );

	const PlanBufs< F > B = plan_bufs< F >( p );
	const int ch = p -> ch;
	const int nv = (int) p -> v.ops.size();
	const int nh = (int) p -> h.ops.size();
	const VRanges R = v_ranges( p -> v, row0, row1 );

	// Horizontal pass over source rows [ya, yb].
	Surf< F > in;
	in.base = (F*) src; in.scan_stride = src_stride; in.idx_stride = ch;
	in.prefix = 0;

	for( int i = 0; i < nh; i++ )
	{
		const LOp& op = p -> h.ops[ i ];
		Surf< F > out;
		out.base = B.hbuf[ i ];
		out.scan_stride = (long) op.out_total * ch;
		out.idx_stride = ch;
		out.prefix = op.out_prefix;

		if(( rc = launch_op( op, ch, true, in, out, R.ya, R.yb + 1, 0,
			op.out_len, st )) != 0 ) return( rc );

		in = out;
	}

	// Vertical pass: scanlines are the NewWidth columns of FltBuf.
	in.base = B.hbuf[ nh - 1 ];
	in.scan_stride = ch;
	in.idx_stride = (long) p -> new_w * ch;
	in.prefix = 0;

	for( int i = 0; i < nv; i++ )
	{
		const LOp& op = p -> v.ops[ i ];
		Surf< F > out;
		out.scan_stride = ch;
		out.idx_stride = (long) p -> new_w * ch;
		out.prefix = op.out_prefix;

		if( i == nv - 1 )
		{
			out.base = dst - (long) row0 * out.idx_stride;
		}
		else
		{
			out.base = B.vbuf[ i ];
		}

		if(( rc = launch_op( op, ch, false, in, out, 0, p -> new_w,
			R.va[ i ], R.vb[ i ] + 1, st )) != 0 ) return( rc );

		in = out;
	}

	return( AVIRHIP_OK );
}

// The source rows [*first, *last] (inclusive) the output rows [row0, row1)
// read: the vertical axis' op chain walked backwards (AVIR), the vertical
// filter positions (LANCIR). Rows outside the range are never touched by a band
// call -- not even by a tap that multiplies them by zero (a stale or foreign
// NaN there must not reach the result; tools/fuzz_values.py poisons them).
void axis_src_range( const LAxis& ax, int row0, int row1, int src_len,
	int* first, int* last )
{
	int a = row0, b = row1 - 1;

	for( int i = (int) ax.ops.size() - 1; i >= 0; i-- )
	{
		int ia, ib;
		const LOp& op = ax.ops[ i ];
		need_range( op, std::max( 0, std::min( a, op.out_len - 1 )),
			std::max( 0, std::min( b, op.out_len - 1 )), ia, ib );
		a = ia;
		b = ib;
	}

	*first = std::max( 0, std::min( a, src_len - 1 ));
	*last = std::max( 0, std::min( b, src_len - 1 ));
}

// (host only: the planner front end answers avirhip_*_band_source_rows for a
// geometry without creating a device plan)
int desc_band_src_rows( const avirhip_plan_desc* d, int row0, int row1,
	int* first, int* last )
{
	LAxis v;
	const int rc = lower_axis( d -> v, d -> src_h, d -> new_h, v,
		d -> work_f64 != 0 );

	if( rc != 0 )
	{
		return( rc );
	}

	axis_src_range( v, row0, row1, d -> src_h, first, last );
	return( AVIRHIP_OK );
}

static void band_src_rows( const avirhip_plan* p, int row0, int row1,
	int* first, int* last )
{
	if( row1 <= row0 )
	{
		*first = 0;
		*last = -1;
		return;
	}

	if( p -> is_lancir )
	{
		*first = std::max( 0, std::min( p -> lv.h_start[ row0 ],
			p -> src_h - 1 ));
		*last = std::max( 0, std::min( p -> lv.h_start[ row1 - 1 ] +
			p -> lv.kernel_len - 1, p -> src_h - 1 ));
		return;
	}

	axis_src_range( p -> v, row0, row1, p -> src_h, first, last );
}

static int band_last_src_row( const avirhip_plan* p, int row0, int row1 )
{
	int a, b;
	band_src_rows( p, row0, row1, &a, &b );
	return( b );
}

// The switch for A/B timing and for tests of the unfused stages: with it, no
// kernel reads the caller's image as it lies and none stores the caller's
// pixels itself -- pack pass and output stage always run. Read once per process.
static bool fused_io()
{
	static const bool on = ( getenv( "AVIRHIP_NO_FUSED_OUT" ) == nullptr );
	return( on );
}

// The line of a stage a call steps aside to, under AVIRHIP_VERBOSE (read per
// call, as the launchers' own lines): "pack pass" -- the float copy of the
// caller's source; "output stage" -- the caller's pixels made from a float
// result. tests/test_gpu_align.py reads the road a call took from them.
static void verbose_stage( const char* const name, const int rows )
{
	if( getenv( "AVIRHIP_VERBOSE" ) != nullptr )
	{
		fprintf( stderr, "%s: %d rows\n", name, rows );
	}
}

// ---- the execute road: AVIR and LANCIR ----

// What belongs to one call. `p` is the plan of the caller's images, `k` the
// plan whose kernels run: `p` itself, or a LANCIR owner's inner float RGBA
// plan. Two things change while the call runs, here and nowhere else. The
// float image the kernels read: the caller's own (float pixels of `k`'s
// channel count, no gamma), or the plan's `packed` copy, which the pack pass
// fills at most once per call and only when a kernel is about to read it
// (road_pack). The float result: the caller's image when `direct`, else the
// plan's `resbuf` (LANCIR: `lres`) -- null until something asked for it.
struct RoadCall
{
	avirhip_plan* p;
	avirhip_plan* k;
	int path;           // of `k`
	ImageRef img;       // the caller's source
	void* dst;          // the caller's result
	int row0, row1;
	hipStream_t st;
	SrcWindow win;
	bool need_pack;     // avir_need_pack; LANCIR: an owner's call
	bool direct;        // avir_direct, LANCIR's `k == p`: `dst` IS the float result
	const float* fsrc;  // the float source, its pitch, ...
	long fstride;
	bool packed;        // ... and whether the pack pass has run for this call
	float* fdst;
};

// A road's attempts: a kernel family and its two sides each (above avir_road)
enum RoadFamily { AVF_DNSRGB, AVF_DN16, AVF_TILES, AVF_UP2, AVF_GPASS,
	AVF_GENERIC, AVF_LANC2H, AVF_LANC2, AVF_LPASS, AVF_LGENERIC };
enum RoadSide { AVS_FLOAT, AVS_RAW, AVS_STORE };
enum RoadFirst { AV1_NOTHING, AV1_SCRATCH, AV1_RESBUF };

struct RoadAttempt
{
	RoadFamily family;
	RoadSide src, res;  // AVS_RAW | AVS_FLOAT, AVS_STORE | AVS_FLOAT
	RoadFirst first;
};

struct Road
{
	int n;
	RoadAttempt a[ 5 ];
	bool lazy, forced;
};

// ---- the road of one LANCIR call (lanc_road). A plain float RGBA plan, unity
// gain, runs its own kernels on the caller's images: every side is FLOAT,
// `direct`, no pack pass; so does any plan forced to path 1, whatever its
// pixels. A plan with integer / scaled / 1-3 channel pixels (the owner) runs
// its inner float RGBA plan's kernels between the pack pass and the output
// stage; where they can, the first reads the owner's image as it lies (RAW)
// and the last runs the owner's output stage in its store (STORE, a
// LancirOut). The float RGBA copy of the source (`packed`) and the float
// result (`lres`) are only allocated when an attempt uses them -- 16 bytes per
// source and per destination pixel, per plan, spare and replica, that also
// count against the plan cache: the automatic path of uint8 / uint16 images
// touches neither. Every row whose condition holds, fastest first:
//
//   attempt        path   sides and condition                            launches
//   k_lanc2h       0, 4   an owner's exact-2x RGBA call, half / bfloat16 k_lanc2h
//                         pixels on a side the kernel may take: RAW 16-bit
//                         / float RGBA | STORE 16-bit, or float of a unity
//                         plan -- images that lanc2h_image_ok takes
//   k_lanc2 raw    4      RAW uint8 / uint16 RGB(A) that lanc2_takes_raw k_lanc2
//                         takes, `dst2`; STORE | FLOAT
//   k_lanc2        4      FLOAT; STORE | FLOAT                           k_lanc2
//   pass raw       5      RAW pixels that gpass_lancir_takes_raw takes   gpass_route's
//                         (16-bit: `io16`); STORE | FLOAT
//   pass           5, 4   FLOAT; STORE | FLOAT. On path 4: the automatic gpass_route's
//                         path alone, when gpass_ok
//   generic        any    FLOAT + FLOAT: the automatic path (and every   launch_lancir_generic
//                         path but 4 and 5)
//
// STORE: an owner's call with `fio` and `out_fast`. A forced path 4 or 5 has
// no generic attempt (`forced`). Every LANCIR road is `lazy`.
static Road lanc_road( const RoadCall& C )
{
	const avirhip_plan* const p = C.p;
	const avirhip_plan* const q = C.k;
	const bool owner = ( q != p );
	const ImageRef& img = C.img;
	const void* const dst = C.dst;
	const int qpath = C.path;
	Road R;

	R.n = 0;
	R.lazy = true;
	R.forced = ( q -> path != 0 && ( qpath == 4 || qpath == 5 ));

	auto add = [&R]( const RoadFamily f, const bool raw, const bool store )
	{
		R.a[ R.n++ ] = RoadAttempt{ f, ( raw ? AVS_RAW : AVS_FLOAT ),
			( store ? AVS_STORE : AVS_FLOAT ), AV1_NOTHING };
	};

	// (double and uint32 elements, lancir.h:373-377: the pack pass and the
	// output stage convert them; the fast kernels' own loaders and fused stores
	// know uint8, uint16 and float)
	// Half and bfloat16 elements: the pass kernels alone know them (path 5:
	// k_lf's and k_gv's raw loaders, kinds 4 / 5; gp_store_lancir_row< 3 > of
	// k_lf and k_gh) -- k_lanc2's loader and fused store do not, so an inner
	// plan on path 4 keeps the pack pass and the output stage around it, also
	// where it falls through to the pass kernels by itself, and every exact-2x
	// plan (q -> lanc2: RGB, RGBA) stays on the roads it had (k_lanc2h below;
	// RGB and integer results behind a 16-bit source: pack pass and output
	// stage), also when path 5 is forced on it. Each
	// side is decided here, once, on its own: the source by the loaders'
	// predicates below, the result by its base address -- elements are stored
	// whole, so an odd base goes through the float result and the output
	// stage. AVIRHIP_GP_NO_IO16 (read per call), as for CImageResizer's pass
	// kernels: both stages for every 16-bit image.
	const bool h_in = dtype_is_float16_kind( p -> in_type );
	const bool h_out = dtype_is_float16_kind( p -> out_type );
	const bool io16 = ( qpath == 5 && q -> lanc2 == nullptr && gpass_io16() );
	const bool in_fast = ( p -> in_type <= AVIRHIP_F32 || ( h_in && io16 ));
	const bool out_fast = ( p -> out_type <= AVIRHIP_F32 || ( h_out && io16 &&
		( (uintptr_t) dst & 1 ) == 0 ));

	// k_lanc2's integer stage behind a raw RGBA source stores a lane's two
	// elements at once
	const bool dst2 = (( p -> io_ch == 3 || ( p -> new_stride & 1 ) == 0 ) &&
		( p -> out_type != AVIRHIP_U8 || p -> io_ch == 3 ||
		( (uintptr_t) dst & 1 ) == 0 ) &&
		( p -> out_type != AVIRHIP_U16 ||
		( (uintptr_t) dst & ( p -> io_ch == 3 ? 1 : 3 )) == 0 ) &&
		( p -> out_type != AVIRHIP_F32 || ( (uintptr_t) dst & 3 ) == 0 ));

	// (AVIRHIP_VARIANT_UP2_UNFUSED_IO: the process-wide switch, per plan)
	const bool fio = ( owner && fused_io() &&
		!( p -> variant & AVIRHIP_VARIANT_UP2_UNFUSED_IO ));
	const bool store = ( fio && out_fast );

	// Exact 2x RGBA with a half / bfloat16 image on either side (lanc2h.hip):
	// one launch, on the automatic path whatever the frame's size (at exact 2x
	// the pass kernels are not offered either type -- `io16` above: behind them
	// the pack pass and the output stage would run) and on forced path 4. A
	// half / bfloat16 RESULT is
	// narrowed and stored by the kernel, whatever the source: the kernel reads
	// a half / bfloat16 / float RGBA source where it lies, the pack pass's
	// float copy of any other. A half / bfloat16 SOURCE with a float result is
	// the kernel's too (the caller's image when the plan is unity, `lres` and
	// the output stage otherwise); with an integer result it is not: that is
	// k_lanc2's fused store behind the pack pass, below. An image that
	// lanc2h_image_ok refuses goes through its float copy, and a call left
	// with float on both sides takes the general road below.
	if( fio && ( h_out || ( h_in && p -> out_type == AVIRHIP_F32 )) &&
		p -> io_ch == 4 && q -> l_order == 4 && q -> lanc2 != nullptr &&
		( p -> path == 0 || p -> path == 4 ))
	{
		const bool src_own = (( h_in || p -> in_type == AVIRHIP_F32 ) &&
			lanc2h_image_ok( img.ptr, p -> in_type, p -> src_stride ));
		const bool dst_own = (( h_out || p -> l_unity ) &&
			lanc2h_image_ok( dst, p -> out_type, p -> new_stride ));

		if(( src_own && h_in ) || ( dst_own && h_out ))
		{
			add( AVF_LANC2H, src_own, dst_own );
		}
	}

	// the inner plan's first pass reads the owner's image itself where it can;
	// otherwise the pack pass makes its float RGBA copy
	if( qpath == 4 )
	{
		if( fio && in_fast && !h_in && lanc2_takes_raw( q, img ) && dst2 )
		{
			add( AVF_LANC2, true, store );
		}

		add( AVF_LANC2, false, store );
	}

	if( qpath == 5 || ( qpath == 4 && q -> path == 0 && gpass_ok( q )))
	{
		// general-ratio pass kernels (vertical pass first)
		// (a raw source on path 5 alone: gpass_lancir_takes_raw asks for it)
		if( fio && in_fast && gpass_lancir_takes_raw( q, img ))
		{
			add( AVF_LPASS, true, store );
		}

		add( AVF_LPASS, false, store );
	}

	if( !R.forced )
	{
		add( AVF_LGENERIC, false, false );
	}

	return( R );
}

// LANCIR's launchers by family, as avir_run_*. STORE: the owner's output stage
static LancirOut lanc_ostage( const RoadCall& C )
{
	const avirhip_plan* const p = C.p;

	return( LancirOut{ C.dst, p -> new_stride, p -> out_type, p -> io_ch,
		p -> l_unity, p -> l_out_mul, p -> l_clamp });
}

static int lanc_run_lanc2h( RoadCall& C, const RoadAttempt& A )
{
	const ImageRef hsrc = ( A.src == AVS_RAW ? C.img : ImageRef{ C.fsrc,
		AVIRHIP_F32, 4, C.fstride });
	const LancirOut hout = ( A.res == AVS_STORE ? lanc_ostage( C ) :
		LancirOut{ C.fdst, (long) C.p -> new_w * 4, AVIRHIP_F32, 4, 1, 1.0f,
		0.0f });

	return( lanc2h_run( C.k, hsrc, hout, C.row0, C.row1, C.st ));
}

static int lanc_run_lanc2( RoadCall& C, const RoadAttempt& A )
{
	const LancirOut ostage = lanc_ostage( C );

	return( lanc2_run( C.k, C.fsrc, C.fdst, C.row0, C.row1, C.st, C.win,
		( A.src == AVS_RAW ? &C.img : nullptr ),
		( A.res == AVS_STORE ? &ostage : nullptr )));
}

static int lanc_run_pass( RoadCall& C, const RoadAttempt& A )
{
	const LancirOut ostage = lanc_ostage( C );

	return( gpass_run( C.k, C.fsrc, C.fstride, C.fdst, C.row0, C.row1, C.st,
		( A.src == AVS_RAW ? &C.img : nullptr ), nullptr,
		( A.res == AVS_STORE ? &ostage : nullptr )));
}

static int lanc_run_generic( RoadCall& C, const RoadAttempt& )
{
	// (the generic kernels' intermediate is only allocated when they run)
	const int rc = ensure_scratch( C.k );

	return( rc != 0 ? rc : launch_lancir_generic( C.k, C.fsrc, C.fdst,
		C.k -> resbuf, C.row0, C.row1, C.st ));
}

// The pack pass, at most once per call: the float copy of the caller's source
// in `k`'s channel count (a LANCIR owner's: float RGBA)
static int road_pack( RoadCall& C )
{
	avirhip_plan* const p = C.p;
	const int ch = C.k -> ch;

	if( !C.need_pack || C.packed )
	{
		return( AVIRHIP_OK );
	}

	C.packed = true;

	// (a lazy call comes here without ensure_scratch; a no-op elsewhere)
	const int ra = need_floats( p, &p -> packed, (size_t) p -> src_w *
		p -> src_h * ch );

	if( ra != 0 ) return( ra );
	C.fsrc = p -> packed;

	// a band converts the source rows its windows read, nothing else (the
	// pipelined host-pointer call is 16 bands: 16 whole-frame packs otherwise)
	int pa, pb;
	band_src_rows( p, C.row0, C.row1, &pa, &pb );

	if( pb < pa )
	{
		return( AVIRHIP_OK );
	}

	const char* const ps = (const char*) C.img.ptr + (size_t) pa *
		p -> src_stride * dtype_size( p -> in_type );
	float* const pd = p -> packed + (size_t) pa * p -> src_w * ch;
	verbose_stage( "pack pass", pb - pa + 1 );

	if( p -> gamma )
	{
		return( launch_pack_gamma( ps, p -> in_type, pd, p -> src_w,
			pb - pa + 1, p -> io_ch, ch, p -> src_stride,
			p -> alpha_index, p -> d_srgb_tbl, C.st ));
	}

	return( launch_pack( ps, p -> in_type, pd, p -> src_w, pb - pa + 1,
		p -> io_ch, ch, p -> src_stride, C.st ));
}

// ---- AVIR ----

// What avir_road asks about a call, beside the plan: the classes of element
// types, whether this call's pixels go through fused loads and stores at all,
// and which results a path's last pass may store itself.
static bool dtype_is_int( const int t )
{
	return( t == AVIRHIP_U8 || t == AVIRHIP_U16 );
}

// (AVIRHIP_VARIANT_UP2_UNFUSED_IO: the process-wide switch, per plan)
static bool avir_fio( const RoadCall& C )
{
	return( fused_io() && !( C.path == 4 &&
		( C.p -> variant & AVIRHIP_VARIANT_UP2_UNFUSED_IO )));
}

// integer / narrow output without gamma / error diffusion: the last pass
// may convert and store into the caller's image itself (no float result,
// no epilogue pass)
// (half / bfloat16 pixels: the marching kernel (4) and the last pass of
// the pass kernels (5, 1-4 channels: gp_store_int_row) narrow and store
// them; behind the tiles the output stage does)
static bool avir_stores( const RoadCall& C )
{
	const avirhip_plan* const p = C.p;

	return( !C.direct && !p -> gamma &&
		(( p -> dither == AVIRHIP_DITHER_DEF && dtype_is_int( p -> out_type )) ||
		p -> out_type == AVIRHIP_F32 ||
		( dtype_is_float16_kind( p -> out_type ) && ( C.path == 4 ||
		( C.path == 5 && gpass_io16() )))) && avir_fio( C ));
}

// this result is the whole-ratio vertical kernel's to store (the two-pass
// tiles, and k_dnfh's integer results): RGBA uint8 pixels are stored whole
static bool avir_dn_stores( const RoadCall& C )
{
	return( avir_stores( C ) && !( C.p -> out_type == AVIRHIP_U8 &&
		C.p -> io_ch == 4 && ( (uintptr_t) C.dst & 3 ) != 0 ) &&
		fused_stores_int( C.p, C.path ));
}

// Path 4 with sRGB gamma: the marching kernel de-linearises and stores a uint8
// result itself (k_up2's IO 8 / 9; up2_stores_io has the plan's conditions).
// AVIRHIP_VARIANT_UP2_UNFUSED_IO and AVIRHIP_NO_FUSED_OUT: the pack pass, the
// float kernel and the output stage, as before these kinds.
static bool up2_gamma_stores( const RoadCall& C )
{
	return( C.path == 4 && C.p -> gamma && !C.direct && avir_fio( C ) &&
		up2_stores_io( C.p ));
}

// The kernel's gamma kinds search the thresholds a row pair at a time (eight
// dependent LDS gathers for a lane's four values), which makes their vertical
// phase about three times the plain kernel's and bound by that latency, where
// the output stage of the road before runs the search at full occupancy. The
// one launch is faster only where the three launches' float traffic outweighs
// that and the frame still fills the chip. Both sides fused (uint8 RGB(A) read
// raw): frames of up2srgb_raw_minpix() to up2srgb_raw_maxpix() source pixels
// (faster at 2,073,600, slower at 921,600 and at 3,686,400: between them the
// interpolated crossings, rounded inwards). The store side alone (the pack
// pass in front) was faster at no size: up to up2srgb_store_maxpix() pixels,
// none by default. AVIRHIP_UP2SRGB_RAW_MINPIX, AVIRHIP_UP2SRGB_RAW_MAXPIX and
// AVIRHIP_UP2SRGB_STORE_MAXPIX, read per call; NOTEBOOK section 34.
static long up2srgb_raw_minpix()
{
	const char* const e = getenv( "AVIRHIP_UP2SRGB_RAW_MINPIX" );

	return( e != nullptr ? atol( e ) : 1700000L );
}

static long up2srgb_raw_maxpix()
{
	const char* const e = getenv( "AVIRHIP_UP2SRGB_RAW_MAXPIX" );

	return( e != nullptr ? atol( e ) : 2700000L );
}

static long up2srgb_store_maxpix()
{
	const char* const e = getenv( "AVIRHIP_UP2SRGB_STORE_MAXPIX" );

	return( e != nullptr ? atol( e ) : 0L );
}

// The store side of k_dnfh's sRGB kinds ALONE (a source the kernel cannot
// read: the pack pass in front of k_dnfh< F32, S8 >) saves the output stage's
// launch and the float result, and pays for the threshold search in the column
// waves, which the DMA-fed row waves no longer hide: it is taken for frames of
// up to dnsrgb_store_maxpix() source pixels (AVIRHIP_DNSRGB_STORE_MAXPIX, read
// per call; measured in NOTEBOOK section 29).
static long dnsrgb_store_maxpix()
{
	const char* const e = getenv( "AVIRHIP_DNSRGB_STORE_MAXPIX" );

	return( e != nullptr ? atol( e ) : 1000000L );
}

// ---- the road of one call (avir_road): decided once, as data, before
// anything is launched or allocated -- the attempts in the order they are
// made. An attempt is a kernel family and its two sides. The source: RAW, the
// first kernel reads the caller's image as it lies, or FLOAT, the caller's
// float image or the pack pass's copy. The result: STORE, the last pass
// converts and stores the caller's pixels at `dst`, or FLOAT, `dst` itself
// when `direct`, else `resbuf` and the output stage. A family's launcher that
// refuses the call (1: alignment, a source window, ...) hands it to the next
// attempt. Per path, every row whose condition holds, in this order:
//
//   attempt        path   condition                                      launches
//   k_dnfh sRGB    2      gamma, 8-bit pixels on a side the kernel may   k_dnfh
//                         take: RAW uint8 RGBA at a base and pitch that
//                         are multiples of 4 | STORE uint8; the store
//                         side alone up to dnsrgb_store_maxpix() pixels
//   k_dnfh 16-bit  2      no gamma, half / bfloat16 pixels on a side the k_dnfh
//                         kernel may take: RAW 16-bit / float RGBA that
//                         lanc2h_image_ok takes | STORE 16-bit at an even
//                         base, integers as the tiles'
//   tiles          2, 3   RAW integer pixels | STORE: avir_dn_stores     k_tile / k_dnf,
//                                                                        dn passes
//   k_up2 raw      4      RAW + STORE: integer RGB(A) or 16-bit RGBA on  k_up2
//                         both sides, up2_stores_io; with gamma uint8
//                         RGB(A) on both sides (the kernel's sRGB kinds),
//                         up2srgb_raw_minpix() to _maxpix() pixels
//   k_up2 store    4      FLOAT + STORE: avir_stores; with gamma a uint8  k_up2
//                         result that up2_stores_io takes (up2_gamma_stores)
//                         up to up2srgb_store_maxpix() pixels
//   k_up2          4      FLOAT + FLOAT                                  k_up2
//   pass store     5      STORE: avir_stores; RAW as below               gpass_route's
//   pass           5      RAW integer / float / 16-bit (`raw16`) pixels  gpass_route's
//                         that gpass_takes_raw takes | FLOAT result
//   generic        any    the automatic path (and every path but 2-5)    run_generic
//
// A forced path 2-5 has no generic attempt: when its last attempt refuses, the
// call ends in AVIRHIP_EUNSUPPORTED (`forced`).
//
// `lazy`: the call skips ensure_scratch and allocates `packed` and `resbuf`
// only when an attempt is about to use them -- k_dnfh's two roads, taken or
// not, k_up2's gamma road, and the pass kernels with 16-bit pixels on a side.
// `first`: what the
// tiles behind k_dnfh, refused or never listed, ask of the plan before they
// make their sides ready: behind the sRGB kinds the float copies their road
// expects to find (ensure_scratch), behind the 16-bit kinds `resbuf` -- also
// where the tiles then store.
static Road avir_road( const RoadCall& C )
{
	const avirhip_plan* const p = C.p;
	const int path = C.path;
	const bool int_in = dtype_is_int( p -> in_type );
	const bool h_in = dtype_is_float16_kind( p -> in_type );
	const bool h_out = dtype_is_float16_kind( p -> out_type );
	const bool dn_fio = ( path == 2 && p -> ch == 4 && fused_io() &&
		!( p -> variant & AVIRHIP_VARIANT_DN_UNFUSED_IO ));
	RoadFirst tiles_first = AV1_NOTHING;
	Road R;

	R.n = 0;
	R.forced = ( p -> path != 0 && path >= 2 && path <= 5 );

	auto add = [&R]( const RoadFamily f, const bool raw, const bool store,
		const RoadFirst first )
	{
		R.a[ R.n++ ] = RoadAttempt{ f, ( raw ? AVS_RAW : AVS_FLOAT ),
			( store ? AVS_STORE : AVS_FLOAT ), first };
	};

	// Whole-ratio downsizing on both axes (path 2) WITH sRGB gamma and 8-bit
	// pixels on a side: k_dnfh's DH_S8 kinds -- one launch that linearises a
	// uint8 RGBA source where it lies (the plan's table) and de-linearises and
	// stores a uint8 result itself (the plan's thresholds; the default
	// ditherer). The sides are independent: `s8` / `o8` say which of them the
	// kernel may take. AVIRHIP_VARIANT_DN_UNFUSED_IO: the tiles' road (pack
	// pass, k_dnf, output stage).
	const bool s8 = ( p -> in_type == AVIRHIP_U8 && p -> io_ch == 4 );
	const bool o8 = ( p -> out_type == AVIRHIP_U8 &&
		p -> dither == AVIRHIP_DITHER_DEF && p -> d_gthr != nullptr );
	const bool srgb = ( dn_fio && p -> gamma && !p -> fp4 && !p -> f64 &&
		( s8 || o8 ) && fused_dn16( p ));

	if( srgb )
	{
		// A source the kernel refuses (a base or a pitch that is no multiple
		// of 4 bytes) or cannot read (RGB, uint16, float) goes through the
		// pack pass's linear copy; a result it cannot store goes as linear
		// float rows. Neither side the kernel's after all: the tiles
		const bool src_own = ( s8 && ( (uintptr_t) C.img.ptr & 3 ) == 0 &&
			( p -> src_stride & 3 ) == 0 );

		if( src_own || ( o8 &&
			(long) p -> src_w * p -> src_h <= dnsrgb_store_maxpix() ))
		{
			add( AVF_DNSRGB, src_own, o8, AV1_NOTHING );
		}

		tiles_first = AV1_SCRATCH;
	}

	// ... with half / bfloat16 pixels on a side, no gamma, the default
	// ditherer: one launch that reads a 16-bit RGBA source where it lies and
	// narrows and stores a 16-bit result itself
	const bool dn16 = ( dn_fio && !p -> gamma &&
		p -> dither == AVIRHIP_DITHER_DEF && ( h_in || h_out ) &&
		fused_dn16( p ));

	if( dn16 )
	{
		// the source k_dnfh reads: the caller's half / bfloat16 / float RGBA
		// image where it lies, the pack pass's float copy of any other (and
		// of one lanc2h_image_ok refuses: a misaligned base, an odd pitch)
		const bool src_own = ( p -> io_ch == 4 && ( h_in || !C.need_pack ) &&
			lanc2h_image_ok( C.img.ptr, p -> in_type, p -> src_stride ));
		// the result: narrowed and stored by the kernel (half / bfloat16),
		// through the integer output stage as k_dnf's, or float rows
		const bool hout = ( !C.direct && ( h_out ?
			( (uintptr_t) C.dst & 1 ) == 0 : avir_dn_stores( C )));

		if(( src_own && p -> in_type != AVIRHIP_F32 ) || ( hout && h_out ))
		{
			add( AVF_DN16, src_own, hout, AV1_NOTHING );
		}

		tiles_first = AV1_RESBUF;
	}

	// (nor does a call of the pass kernels with 16-bit pixels on a side, whose
	// first pass may read and whose last pass may store them, make its float
	// copies up front)
	// (nor does the marching kernel's gamma road: a uint8 call that the raw kind
	// completes holds neither copy)
	// (with gamma: a uint8 RGB(A) image through the linearising table and the
	// uint8 result through the thresholds; or the thresholds alone)
	const long up2g_px = (long) p -> src_w * p -> src_h;
	const bool up2g_any = up2_gamma_stores( C );
	const bool up2g_raw = ( up2g_any && p -> ch == 4 &&
		p -> in_type == AVIRHIP_U8 && p -> d_srgb_tbl != nullptr &&
		up2g_px >= up2srgb_raw_minpix() && up2g_px <= up2srgb_raw_maxpix());
	const bool up2g_store = ( up2g_any && up2g_px <= up2srgb_store_maxpix());
	const bool up2g = ( up2g_raw || up2g_store );

	R.lazy = ( srgb || dn16 || up2g || ( path == 5 && !p -> gamma &&
		gpass_io16() && ( h_in || h_out )));

	// integer / narrower sources: the path's first kernel reads the caller's
	// image as it lies, the float copy of the source (pack pass) is skipped --
	// the tile loaders (2, 3), the streaming pass kernel (5), and the marching
	// kernel (4) when it also stores the caller's integer pixels (it may still
	// refuse the call -- alignment, a source window: the pack pass runs then)
	const bool raw_ok = ( !p -> gamma && p -> ch == 4 );

	if( path == 2 || path == 3 )
	{
		add( AVF_TILES, raw_ok && int_in && fused_takes_raw( p, path ),
			avir_dn_stores( C ), tiles_first );
	}

	if( path == 4 )
	{
		// half RGBA on both sides, or bfloat16 RGBA on both sides: the marching
		// kernel reads the elements as they lie
		const bool half_io = ( h_in && p -> out_type == p -> in_type &&
			p -> io_ch == 4 );
		const bool stores = ( avir_stores( C ) || up2g_store );

		// (up2g_raw: up2_stores_io, the default ditherer and avir_fio hold;
		// up2_run may still refuse -- a source window, AVIRHIP_UP2_NO_RAW: the
		// next row, or the road before when the store side alone is not offered)
		if(( up2g_raw || ( stores && raw_ok )) && C.need_pack && (( int_in &&
			( p -> io_ch == 3 || p -> io_ch == 4 ) &&
			dtype_is_int( p -> out_type )) || half_io ) &&
			p -> dither == AVIRHIP_DITHER_DEF && up2_stores_io( p ) &&
			avir_fio( C ))
		{
			add( AVF_UP2, true, true, AV1_NOTHING ); // (no pack pass, no epilogue)
		}

		if( stores )
		{
			add( AVF_UP2, false, true, AV1_NOTHING );
		}

		add( AVF_UP2, false, false, AV1_NOTHING );
	}

	if( path == 5 )
	{
		// a half / bfloat16 source k_gh's typed loader takes: elements
		// are loaded whole, four at a time -- a base that is a multiple of their
		// size, at least four of them up to the end of the last source row the
		// band's first pass reads (run_h's `raw_elems`); any row pitch. The
		// accumulation kernels' typed loaders (a horizontal axis with k >= 2,
		// gpass.hip: sa16_wanted, asked through gpass_takes_raw) take the same
		const bool raw16 = ( gpass_io16() && h_in &&
			( (uintptr_t) C.img.ptr & 1 ) == 0 && C.row1 > C.row0 &&
			(long) gpass_last_src_row( p, C.row0, C.row1 ) * p -> src_stride +
			(long) p -> src_w * p -> io_ch >= 4 );
		const bool raw = ( raw_ok && C.need_pack &&
			( int_in || p -> in_type == AVIRHIP_F32 || raw16 ) &&
			gpass_takes_raw( p ));

		if( avir_stores( C ))
		{
			add( AVF_GPASS, raw, true, AV1_NOTHING );
		}

		// (this plan's last pass cannot: float result)
		add( AVF_GPASS, raw, false, AV1_NOTHING );
	}

	if( !R.forced )
	{
		add( AVF_GENERIC, false, false, AV1_NOTHING );
	}

	return( R );
}

// the float result buffer of a call that is not `direct`: `resbuf`, a LANCIR
// owner's `lres` ...
static float*& road_res( const RoadCall& C )
{
	return( C.p -> is_lancir ? C.p -> lres : C.p -> resbuf );
}

// ... when it is needed
static int road_need_res( const RoadCall& C )
{
	return( C.direct ? AVIRHIP_OK : need_floats( C.p, &road_res( C ),
		(size_t) C.p -> new_w * C.p -> new_h * C.k -> ch ));
}

// ---- one function per family: its launcher, with the sides of the attempt.
// Each returns the launcher's code -- 1: it cannot take this call.
static int avir_run_dnfh( RoadCall& C, const RoadAttempt& A )
{
	const ImageRef hsrc = ( A.src == AVS_RAW ? C.img : ImageRef{ C.fsrc,
		AVIRHIP_F32, 4, C.fstride });
	void* const hout = ( A.res == AVS_STORE ? C.dst : nullptr );

	return( A.family == AVF_DNSRGB ?
		fused_run_dnsrgb( C.p, hsrc, C.fdst, C.row0, C.row1, C.st, hout ) :
		fused_run_dn16( C.p, hsrc, C.fdst, C.row0, C.row1, C.st, hout ));
}

static int avir_run_tiles( RoadCall& C, const RoadAttempt& A )
{
	avirhip_plan* const p = C.p;
	void* const iout = ( A.res == AVS_STORE ? C.dst : nullptr );

	return( A.src == AVS_RAW ?
		fused_run( p, C.path, C.img.ptr, p -> in_type, p -> io_ch,
		p -> src_stride, C.fdst, C.row0, C.row1, C.st, iout ) :
		fused_run( p, C.path, C.fsrc, AVIRHIP_F32, 4, C.fstride, C.fdst,
		C.row0, C.row1, C.st, iout ));
}

static int avir_run_up2( RoadCall& C, const RoadAttempt& A )
{
	if( A.res == AVS_STORE )
	{
		return( A.src == AVS_RAW ?
			up2_run( C.p, nullptr, 0, nullptr, C.row0, C.row1, C.st, C.win,
			&C.img, C.dst ) :
			up2_run( C.p, C.fsrc, C.fstride, nullptr, C.row0, C.row1, C.st,
			C.win, nullptr, C.dst ));
	}

	return( up2_run( C.p, C.fsrc, C.fstride, C.fdst, C.row0, C.row1, C.st,
		C.win, nullptr, nullptr ));
}

static int avir_run_gpass( RoadCall& C, const RoadAttempt& A )
{
	void* const iout = ( A.res == AVS_STORE ? C.dst : nullptr );

	return( A.src == AVS_RAW ?
		gpass_run( C.p, nullptr, 0, C.fdst, C.row0, C.row1, C.st, &C.img, iout,
		nullptr ) :
		gpass_run( C.p, C.fsrc, C.fstride, C.fdst, C.row0, C.row1, C.st,
		nullptr, iout, nullptr ));
}

static int avir_run_generic( RoadCall& C, const RoadAttempt& )
{
	return( run_generic( C.p, C.fsrc, C.fstride, C.fdst, C.row0, C.row1,
		C.st ));
}

// The tail of a call whose float result is at `fdst` (and is not the caller's
// image): the owner's output stage (LANCIR), error diffusion or the output
// stage (AVIR) into `dst`.
static int road_output( const RoadCall& C )
{
	avirhip_plan* const p = C.p;
	const float* const fdst = C.fdst;
	void* const dst = C.dst;
	const int row0 = C.row0, row1 = C.row1;
	const hipStream_t st = C.st;

	verbose_stage( "output stage", row1 - row0 );

	if( p -> is_lancir )
	{
		return( p -> io_ch == 4 ?
			launch_lancir_out( p, fdst, (long) p -> new_w * 4, dst, row1 - row0,
			st ) : launch_lancir_out_pad( p, fdst, dst, row1 - row0, st ));
	}

	if( p -> dither == AVIRHIP_DITHER_ERRD )
	{
		// recursive ditherer: whole frames only (exec_any refuses bands).
		// One row of diffusion values per pass of 448 rows (generic.hip:
		// k_errd_mp; the single-workgroup kernels use two), then the passes'
		// progress flags
		if( p -> errd_line == nullptr )
		{
			void* q;
			const size_t np = (size_t) ( p -> new_h + 447 ) / 448 + 2;
			const int rc = dev_alloc( p, np * p -> new_w * 4 * sizeof( float ) +
				np * sizeof( unsigned ) + 64, &q );

			if( rc != 0 ) return( rc );
			p -> errd_line = (float*) q;
		}

		return( launch_errd( fdst, dst, p -> out_type, p -> new_w, p -> new_h,
			p -> io_ch, p -> ch, p -> tr_mul, p -> pk_out, p -> gamma,
			p -> alpha_index, p -> errd_line, st ));
	}

	return( launch_epilogue( fdst, dst, p -> out_type,
		(long) ( row1 - row0 ) * p -> new_w * p -> io_ch, p -> tr_mul,
		p -> pk_out, ( p -> gamma && (( p -> out_type != AVIRHIP_F32 &&
		!dtype_is_float16_kind( p -> out_type )) || p -> fp4 )), p -> io_ch,
		p -> ch, p -> alpha_index, st,
		p -> d_gthr, ( p -> dither == AVIRHIP_DITHER_DEF_RNE )));
}

// The attempts of a road in turn, each with its sides made ready, until one
// does not refuse the call; then the output stage, unless the last pass stored
// the caller's pixels or the caller's image is the float result.
static int road_execute( RoadCall& C, const Road& R )
{
	static int ( * const run[] )( RoadCall&, const RoadAttempt& ) = {
		avir_run_dnfh, avir_run_dnfh, avir_run_tiles, avir_run_up2,
		avir_run_gpass, avir_run_generic, lanc_run_lanc2h, lanc_run_lanc2,
		lanc_run_pass, lanc_run_generic }; // (by RoadFamily)
	avirhip_plan* const p = C.p;
	bool stored = false;
	int rc = 1;

	for( int i = 0; i < R.n && rc == 1; i++ )
	{
		const RoadAttempt& A = R.a[ i ];

		if( A.first == AV1_SCRATCH && ( rc = ensure_scratch( p )) != 0 )
			return( rc );

		if( A.first == AV1_RESBUF && ( rc = road_need_res( C )) != 0 )
			return( rc );

		// (the pack before the result buffer of the same attempt)
		if( A.src == AVS_FLOAT && ( rc = road_pack( C )) != 0 ) return( rc );
		if( A.res == AVS_FLOAT && ( rc = road_need_res( C )) != 0 ) return( rc );

		C.fdst = ( C.direct ? (float*) C.dst : road_res( C ));
		rc = run[ A.family ]( C, A );
		stored = ( rc == 0 && A.res == AVS_STORE );
	}

	if( rc == 1 && R.forced )
	{
		set_error( "path %d cannot run this call (unaligned buffers?)",
			C.path );
		return( AVIRHIP_EUNSUPPORTED );
	}

	if( rc != 0 || stored || C.direct )
	{
		return( rc ); // (no epilogue)
	}

	return( road_output( C ));
}

static int exec_avir( avirhip_plan* p, const void* src, void* dst, int row0,
	int row1, hipStream_t st, const SrcWindow win )
{
	RoadCall C;
	C.p = p;
	C.k = p;
	C.path = ( p -> path != 0 ? p -> path : p -> auto_path );
	C.img = ImageRef{ src, p -> in_type, p -> io_ch, p -> src_stride };
	C.dst = dst;
	C.row0 = row0; C.row1 = row1;
	C.st = st;
	C.win = win;
	C.need_pack = avir_need_pack( p );
	C.direct = avir_direct( p );
	C.fsrc = ( C.need_pack ? nullptr : (const float*) src );
	C.fstride = ( C.need_pack ? (long) p -> src_w * p -> ch :
		(long) p -> src_stride );
	C.packed = false;
	C.fdst = nullptr;

	const Road R = avir_road( C );

	// (a lazy road makes neither float copy: road_pack and road_need_res
	// allocate them where an attempt needs them after all)
	const int rc = ( R.lazy ? AVIRHIP_OK : ensure_scratch( p ));

	return( rc != 0 ? rc : road_execute( C, R ));
}

// A LANCIR call. The owner: a plan with an inner plan, unless it is forced to
// path 1 (its own generic kernels, whatever its pixels). `win` is a plain
// plan's alone, and k_lanc2's.
static int exec_lancir( avirhip_plan* p, const void* src, void* dst, int row0,
	int row1, hipStream_t st, const SrcWindow win )
{
	const bool owner = ( p -> inner != nullptr && p -> path != 1 );

	if( owner && row1 <= row0 )
	{
		return( AVIRHIP_OK );
	}

	RoadCall C;
	C.p = p;
	C.k = ( owner ? p -> inner : p );
	C.path = ( C.k -> path != 0 ? C.k -> path : C.k -> auto_path );
	C.img = ImageRef{ src, p -> in_type, p -> io_ch, p -> src_stride };
	C.dst = dst;
	C.row0 = row0; C.row1 = row1;
	C.st = st;
	C.win = ( owner ? SrcWindow{ 0, 0 } : win );
	C.need_pack = owner;
	C.direct = !owner;
	// (a raw source's kernels are handed the float copy of an earlier call, or
	// none: they do not read it)
	C.fsrc = ( owner ? p -> packed : (const float*) src );
	C.fstride = C.k -> src_stride;
	C.packed = false;
	C.fdst = nullptr;

	return( road_execute( C, lanc_road( C )));
}

// One call on device-resident buffers, by route.
// `win`: a native source window (exec_any) -- `src` is then the virtual frame
// base of the marching kernels, which are the only kernels such a call reaches
static int exec_device( avirhip_plan* p, const void* src, void* dst,
	int row0, int row1, hipStream_t st, const SrcWindow win )
{
	if( p -> f64 )
	{
		return( exec_f64( p, src, dst, row0, row1, st ));
	}

	return( p -> is_lancir ? exec_lancir( p, src, dst, row0, row1, st, win ) :
		exec_avir( p, src, dst, row0, row1, st, win ));
}

// the per-op executor of the double pipeline (generic64.hip: exec_f64)
template int ensure_generic_scratch< double >( avirhip_plan* );
template int run_generic< double >( avirhip_plan*, const double*, long,
	double*, int, int, hipStream_t );

} // namespace avirhip

// AVIRHIP_MEM_AUTO: device memory if the HIP runtime knows the pointer as such.
extern "C" int avirhip_resolve_mem( const void* ptr, int mem )
{
	if( mem != AVIRHIP_MEM_AUTO )
	{
		return( mem );
	}

	hipPointerAttribute_t at;

	if( ptr != nullptr && hipPointerGetAttributes( &at, ptr ) == hipSuccess &&
		( at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged ))
	{
		return( AVIRHIP_MEM_DEVICE );
	}

	(void) hipGetLastError(); // unregistered host memory reports an error
	return( AVIRHIP_MEM_HOST );
}

namespace avirhip {

static int clone_plan( const avirhip_plan* s, int device, avirhip_plan** out );

// The copy streams and the 2 * nb + 1 events of the band pipeline, made when a
// plan's first pipelined call needs them: built aside and committed to the
// plan only when complete -- a plan must never hold half a set (the next call
// would index past pipe_ev). false: they could not be made.
static bool ensure_pipe_set( avirhip_plan* p, const int nb )
{
	if( p -> pipe_in != nullptr )
	{
		return( true );
	}

	hipStream_t a = nullptr, b = nullptr;
	std::vector< hipEvent_t > evs;
	bool ok = ( hipStreamCreateWithFlags( &a, hipStreamNonBlocking ) ==
		hipSuccess );

	ok = ok && ( hipStreamCreateWithFlags( &b, hipStreamNonBlocking ) ==
		hipSuccess );

	for( int i = 0; ok && i < 2 * nb + 1; i++ )
	{
		hipEvent_t e;
		ok = ( hipEventCreateWithFlags( &e, hipEventDisableTiming ) ==
			hipSuccess );

		if( ok ) evs.push_back( e );
	}

	if( !ok )
	{
		(void) hipGetLastError();

		for( size_t i = 0; i < evs.size(); i++ )
		{
			(void) hipEventDestroy( evs[ i ]);
		}

		if( a != nullptr ) (void) hipStreamDestroy( a );
		if( b != nullptr ) (void) hipStreamDestroy( b );

		return( false );
	}

	p -> pipe_in = a; p -> pipe_out = b;
	p -> pipe_ev.swap( evs );
	return( true );
}

// Host-pointer call, pipelined (the call every existing caller of the
// reference makes, avir.h:4680-4684): the frame in row bands, the source rows
// of band b + 1 travelling host -> device (an uploader thread: a copy from
// pageable memory holds its thread until the data is staged) while band b is
// computed and band b - 1 travels device -> host. PCIe is full duplex, so the
// call costs the longer direction instead of the sum (cfg3: 531 MB down,
// 133 MB up). Returns 1 when the call should take the serial path.
static int exec_host_pipelined( avirhip_plan* p, const void* src, void* dst,
	size_t src_bytes, size_t dst_bytes, size_t row_bytes, hipStream_t st )
{
	static const bool off = ( getenv( "AVIRHIP_NO_HOST_PIPELINE" ) != nullptr );
	enum { NBMAX = 32 };
	static const int NB = []() { const char* e = getenv( "AVIRHIP_HOST_BANDS" );
		const int n = ( e != nullptr ? atoi( e ) : 16 );
		return( n < 2 ? 2 : ( n > NBMAX ? (int) NBMAX : n )); }();

	// Every band is one exec_device call. Stages that are not limited to the
	// band's rows would be repeated NB times: the double pipeline and the
	// generic kernels run whole axes through a filtered upsample -- such calls
	// stay serial. (The pack pass converts only the rows a band reads.)
	const int xp = ( p -> path != 0 ? p -> path : p -> auto_path );

	if( p -> f64 || ( !p -> is_lancir && xp == 1 ))
	{
		return( 1 );
	}

	if( off || p -> new_h < 4 * NB || src_bytes + dst_bytes < ( 16u << 20 ) ||
		( !p -> is_lancir && p -> dither == AVIRHIP_DITHER_ERRD &&
		( p -> out_type == AVIRHIP_U8 || p -> out_type == AVIRHIP_U16 )))
	{
		return( 1 );
	}

	if( !ensure_pipe_set( p, NB ))
	{
		return( 1 ); // (the serial path needs none of this)
	}

	hipStream_t s_in = (hipStream_t) p -> pipe_in;
	hipStream_t s_out = (hipStream_t) p -> pipe_out;
	static const bool do_reg = ( getenv( "AVIRHIP_HOST_REGISTER" ) != nullptr );
	bool reg_s = false, reg_d = false;

	if( do_reg )
	{
		reg_s = ( hipHostRegister( (void*) src, src_bytes,
			hipHostRegisterDefault ) == hipSuccess );
		reg_d = ( hipHostRegister( dst, dst_bytes, hipHostRegisterDefault ) ==
			hipSuccess );
		(void) hipGetLastError();
	}

	const size_t es = dtype_size( p -> in_type );
	const size_t srow = (size_t) p -> src_stride * es;
	int cut[ NBMAX + 1 ], last[ NBMAX ];

	for( int b = 0; b <= NB; b++ )
	{
		cut[ b ] = (int) ( (long) p -> new_h * b / NB );
	}

	for( int b = 0; b < NB; b++ )
	{
		last[ b ] = band_last_src_row( p, cut[ b ], cut[ b + 1 ]);

		if( b > 0 )
		{
			last[ b ] = std::max( last[ b ], last[ b - 1 ]);
		}
	}

	last[ NB - 1 ] = p -> src_h - 1;

	// the copy streams start behind whatever the caller's stream holds
	hipEvent_t e0 = p -> pipe_ev[ 2 * NB ];
	AVIRHIP_HIPCHECK( hipEventRecord( e0, st ));
	AVIRHIP_HIPCHECK( hipStreamWaitEvent( s_in, e0, 0 ));
	AVIRHIP_HIPCHECK( hipStreamWaitEvent( s_out, e0, 0 ));

	std::atomic< int > ready( -1 );
	std::atomic< int > up_err( 0 );
	const int dev = p -> device;
	char* const dsrc = (char*) p -> stage_src;

	auto upload_rows = [&]()
	{
		hipError_t he = hipSetDevice( dev );

		if( he != hipSuccess )
		{
			up_err.store( (int) he );
			ready.store( NB );
			return;
		}

		int done = 0; // source rows on their way

		for( int b = 0; b < NB; b++ )
		{
			const int upto = last[ b ] + 1;

			if( upto > done )
			{
				const size_t o0 = (size_t) done * srow;
				const size_t o1 = std::min( src_bytes, (size_t) upto * srow );

				if( o1 > o0 && ( he = hipMemcpyAsync( dsrc + o0,
					(const char*) src + o0, o1 - o0, hipMemcpyHostToDevice,
					s_in )) != hipSuccess )
				{
					up_err.store( (int) he );
				}

				done = upto;
			}

			if(( he = hipEventRecord( p -> pipe_ev[ b ], s_in )) != hipSuccess )
			{
				up_err.store( (int) he );
			}

			ready.store( b );
		}
	};

	// (a thread that cannot be started must not throw through extern "C":
	// the rows then go up from this thread, band after band, before the loop)
	// (... and a throw below -- a host allocation failing inside a band's launch
	// code -- must not unwind past a joinable thread: that is std::terminate)
	struct Joiner
	{
		std::thread t;
		~Joiner() { if( t.joinable() ) t.join(); }
	} up;
	std::thread& uploader = up.t;

	try
	{
		uploader = std::thread( upload_rows );
	}
	catch( ... )
	{
		upload_rows();
	}

	int rc = AVIRHIP_OK;

	// band b's copy down holds this thread (pageable memory), so band b + 1's
	// kernels are enqueued BEFORE it: the device never waits for the host
	auto copy_down = [&]( const int b )
	{
		const size_t off_b = (size_t) cut[ b ] * row_bytes;
		const size_t len_b = std::min( dst_bytes,
			(size_t) cut[ b + 1 ] * row_bytes ) - off_b;

		if( hipStreamWaitEvent( s_out, p -> pipe_ev[ NB + b ], 0 ) != hipSuccess ||
			hipMemcpyAsync( (char*) dst + off_b, (char*) p -> stage_dst + off_b,
			len_b, hipMemcpyDeviceToHost, s_out ) != hipSuccess )
		{
			rc = AVIRHIP_EHIP;
		}
	};

	int enq = 0; // bands whose kernels are enqueued

	for( int b = 0; b < NB && rc == AVIRHIP_OK; b++ )
	{
		while( ready.load() < b )
		{
			std::this_thread::yield();
		}

		if( up_err.load() != 0 )
		{
			break;
		}

		if( hipStreamWaitEvent( st, p -> pipe_ev[ b ], 0 ) != hipSuccess )
		{
			rc = AVIRHIP_EHIP;
			break;
		}

		rc = exec_device( p, dsrc, (char*) p -> stage_dst +
			(size_t) cut[ b ] * row_bytes, cut[ b ], cut[ b + 1 ], st,
			SrcWindow{ 0, 0 });

		if( rc != AVIRHIP_OK )
		{
			break;
		}

		if( hipEventRecord( p -> pipe_ev[ NB + b ], st ) != hipSuccess )
		{
			rc = AVIRHIP_EHIP;
			break;
		}

		enq = b + 1;

		if( b >= 1 )
		{
			copy_down( b - 1 );
		}
	}

	if( rc == AVIRHIP_OK && enq == NB )
	{
		copy_down( NB - 1 );
	}

	if( uploader.joinable() ) uploader.join();
	(void) hipStreamSynchronize( s_in );
	(void) hipStreamSynchronize( s_out );
	(void) hipStreamSynchronize( st );

	if( reg_s ) (void) hipHostUnregister( (void*) src );
	if( reg_d ) (void) hipHostUnregister( dst );

	if( up_err.load() != 0 && rc == AVIRHIP_OK )
	{
		set_error( "host-pointer call: the source upload failed: %s",
			hipGetErrorString( (hipError_t) up_err.load() ));
		rc = AVIRHIP_EHIP;
	}

	return( rc );
}


// ---- the execute entry: every whole-frame, band, window, sharded and timed
// call is one exec_any, which is a sequence of the stages below

// bytes behind an image of `rows` rows at a pitch of `stride` elements: the
// last row ends with its last pixel
static size_t image_bytes( int rows, long stride, int w, int ch, int type )
{
	return(( (size_t) ( rows - 1 ) * stride + (size_t) w * ch ) *
		dtype_size( type ));
}

static bool share_bytes( const void* a, size_t na, const void* b, size_t nb )
{
	return( (const char*) a < (const char*) b + nb &&
		(const char*) b < (const char*) a + na );
}

// The caller's current device, put back on every way out. `want` >= 0: a
// plan's tables and scratch live on the device it was created on -- the call
// runs there, whatever device the calling thread has current (and the caller's
// device is put back only if it was left).
struct DeviceGuard
{
	int keep;
	bool on;
	explicit DeviceGuard( int want = -1 ) : keep( 0 ), on( want < 0 )
	{
		if( hipGetDevice( &keep ) == hipSuccess && want >= 0 && keep != want )
		{
			on = ( hipSetDevice( want ) == hipSuccess );
		}
	}
	~DeviceGuard() { if( on ) (void) hipSetDevice( keep ); }
};

// The argument, window and band checks of a call. `nothing`: the call is valid
// and has no row to compute.
static int check_call( const avirhip_plan* p, const void* src, const void* dst,
	int row0, int row1, int win_first, int win_rows, bool& nothing )
{
	nothing = false;

	if( p == nullptr || src == nullptr || dst == nullptr || row0 < 0 ||
		row1 > p -> new_h || row0 > row1 )
	{
		set_error( "bad execute arguments" );
		return( AVIRHIP_EINVAL );
	}

	if( win_rows > 0 )
	{
		int need_a = 0, need_b = -1;
		band_src_rows( p, row0, row1, &need_a, &need_b );

		// (compared in long: win_first + win_rows of a hostile caller must not
		// wrap; the window has to lie inside the frame whatever the band reads)
		if( win_first < 0 || (long) win_first + win_rows > (long) p -> src_h ||
			( need_b >= need_a && ( need_a < win_first ||
			(long) need_b >= (long) win_first + win_rows )))
		{
			set_error( "resize_window: output rows [%d, %d) read source rows "
				"[%d, %d], the window holds [%d, %d)", row0, row1, need_a,
				need_b, win_first, win_first + win_rows );
			return( AVIRHIP_EINVAL );
		}

		// an empty band reads nothing and stores nothing: done before any copy
		// of the window is made
		if( row1 <= row0 )
		{
			nothing = true;
			return( AVIRHIP_OK );
		}
	}

	if( !p -> is_lancir && p -> dither == AVIRHIP_DITHER_ERRD &&
		( row0 != 0 || row1 != p -> new_h ))
	{
		set_error( "the error-diffusion ditherer is recursive over rows "
			"(avir.h:4473-4480): row bands cannot be executed" );
		return( AVIRHIP_EUNSUPPORTED );
	}

	return( AVIRHIP_OK );
}

// The plan a scratch-using call runs on, its lock in `held` (released on every
// way out of the caller, a throw included). Scratch users take the plan's lock.
// When another thread holds it (the reference allows concurrent resizeImage()
// calls on one object, README.md:83-85), the call runs on a spare replica of
// the plan instead -- same tables, its own scratch, staging buffers and last_*
// state -- so that the two calls overlap on their streams rather than queue
// behind one buffer set. Up to three spares; beyond that callers wait.
static avirhip_plan* scratch_owner( avirhip_plan* p,
	std::unique_lock< std::mutex >& held )
{
	held = std::unique_lock< std::mutex >( p -> exec_mtx, std::try_to_lock );

	if( held.owns_lock() )
	{
		return( p );
	}

	avirhip_plan* spare = nullptr;
	{
		// (its own mutex: avirhip_resize_sharded holds shard_mtx for the
		// whole call and reaches this point for the band on the plan's
		// own device)
		std::lock_guard< std::mutex > sl( p -> spare_mtx );

		for( size_t i = 0; i < p -> spares.size() && spare == nullptr; i++ )
		{
			if( p -> spares[ i ] -> exec_mtx.try_lock())
			{
				spare = p -> spares[ i ];
			}
		}

		if( spare == nullptr && p -> spares.size() < 3 && !p -> is_spare )
		{
			if( clone_plan( p, p -> device, &spare ) == AVIRHIP_OK )
			{
				spare -> is_spare = 1;
				spare -> exec_mtx.lock();
				p -> spares.push_back( spare );
			}
			else
			{
				spare = nullptr;
			}
		}
	}

	if( spare != nullptr )
	{
		held = std::unique_lock< std::mutex >( spare -> exec_mtx,
			std::adopt_lock );
		return( spare );
	}

	held.lock();
	return( p );
}

// hipStreamPerThread is ONE handle that names a different stream in every
// thread: such a call records the plan's event itself, when it ends.
struct PerThreadRecord
{
	avirhip_plan* p;
	hipStream_t st;
	bool on;
	~PerThreadRecord()
	{
		if( on && ( p -> last_done == nullptr ||
			hipEventRecord( p -> last_done, st ) != hipSuccess ))
		{
			(void) hipGetLastError();
			(void) hipStreamSynchronize( st );
		}
	}
};

// The plan's scratch buffers are reused by the next call. Calls on one
// stream are ordered by the stream itself; only when the stream
// CHANGES does the new one have to wait for what the old one still
// holds -- the event is recorded on the old stream then, not after
// every call: a record between two frames is a barrier packet with a
// release fence, 6-8 us of idle GPU per frame (the kernel trace of
// 640x480 -> 1024x768: H -> V inside a call 0.6 us apart, V -> the next
// call's H 7.7 us). "The same stream" is the same handle AND, for
// hipStreamPerThread, the same thread. (hipStreamGetId would also tell a
// destroyed stream's recycled handle value apart, but it is a hip_7.1
// symbol: the runtime PyTorch ships is 7.0 and could not load the
// library. A caller that destroys a stream with calls of this plan
// still in flight has to synchronise it first.)
// `record_at_end`: the caller's PerThreadRecord is armed.
static int order_behind_last_call( avirhip_plan* p, hipStream_t st,
	bool& record_at_end )
{
	const bool per_thread = ( st == hipStreamPerThread );
	const std::thread::id tid = std::this_thread::get_id();

	if( p -> last_used )
	{
		if( p -> last_done == nullptr )
		{
			AVIRHIP_HIPCHECK( hipEventCreateWithFlags( &p -> last_done,
				hipEventDisableTiming ));
		}

		if( p -> last_recorded )
		{
			// (the last call was on a per-thread stream and recorded the
			// event when it ended)
			if( !( per_thread && p -> last_tid == tid ))
			{
				AVIRHIP_HIPCHECK( hipStreamWaitEvent( st, p -> last_done, 0 ));
			}
		}
		else
		if( p -> last_stream != (void*) st )
		{
			if( hipEventRecord( p -> last_done,
				(hipStream_t) p -> last_stream ) != hipSuccess ||
				hipStreamWaitEvent( st, p -> last_done, 0 ) != hipSuccess )
			{
				// (the old stream is gone: what it held may still run)
				(void) hipGetLastError();
				AVIRHIP_HIPCHECK( hipDeviceSynchronize() );
			}
		}
	}
	else
	if( per_thread && p -> last_done == nullptr )
	{
		AVIRHIP_HIPCHECK( hipEventCreateWithFlags( &p -> last_done,
			hipEventDisableTiming ));
	}

	p -> last_stream = (void*) st;
	p -> last_tid = tid;
	p -> last_recorded = per_thread;
	p -> last_used = true;
	record_at_end = per_thread;
	return( AVIRHIP_OK );
}

// Where the kernels of one call read the source from, and which bytes move
// before they do:
//   call                                      stage_src  copy            kernels read     window
//   device frame, no bytes shared with dst    --         --              src              --
//   device frame sharing bytes with dst       frame      frame, D2D      stage            --
//   host frame                                frame      frame, H2D, late  stage          --
//   window, marching kernel, device, apart    --         --              src - win_off    yes
//   window, marching kernel, host or shared   window     window to 0     stage - win_off  yes
//   window, any other plan                    frame      window to win_off  stage         --
struct SrcRoute
{
	size_t stage_bytes; // what stage_src has to hold (0: `src` is read where it lies)
	size_t copy_bytes;  // bytes of `src` copied there (0: none) ...
	size_t copy_at;     // ... to this offset of stage_src ...
	hipMemcpyKind kind;
	bool late;          // ... only after the band pipeline has declined the call
	size_t base_off;    // subtracted from the buffer: the virtual frame base
	SrcWindow win;      // the kernels' row clamp: an argument of this call
};

static SrcRoute src_route( const avirhip_plan* p, const void* src, int src_mem,
	const void* dst, int dst_mem, int row0, int row1, int win_first,
	int win_rows )
{
	const bool windowed = ( win_rows > 0 );
	const bool host = ( src_mem == AVIRHIP_MEM_HOST );
	const size_t src_bytes = image_bytes( p -> src_h, p -> src_stride,
		p -> src_w, p -> io_ch, p -> in_type );
	// (what `src` addresses: the frame, or the rows of a window)
	const size_t win_bytes = ( !windowed ? src_bytes : image_bytes( win_rows,
		p -> src_stride, p -> src_w, p -> io_ch, p -> in_type ));
	const size_t dst_bytes = ( row1 > row0 ? image_bytes( row1 - row0,
		p -> new_stride, p -> new_w, p -> io_ch, p -> out_type ) : 0 );
	const bool shared = ( src_mem == AVIRHIP_MEM_DEVICE &&
		dst_mem == AVIRHIP_MEM_DEVICE &&
		share_bytes( src, win_bytes, dst, dst_bytes ));
	SrcRoute r = { 0, 0, 0, ( host ? hipMemcpyHostToDevice :
		hipMemcpyDeviceToDevice ), false, 0, { 0, 0 }};

	if( !windowed )
	{
		// NewBuf may alias SrcBuf (avir.h:4650-4652: allowed when the result is
		// not larger). The reference survives that because it has consumed the
		// source into FltBuf before it writes; the kernels here read the source
		// while they write, so an overlapping device source is copied aside first.
		if( host || shared )
		{
			r.stage_bytes = r.copy_bytes = src_bytes;
			r.late = host;
		}

		return( r );
	}

	// A window on the marching kernels (exact-2x float RGBA plans: the sharded
	// configurations of BASELINE.json): the kernels take a VIRTUAL frame base,
	// window - win_first rows, and clamp their row indices to the window -- for
	// every access that reaches a result "clamp to the window" IS "clamp to the
	// frame" (a needed row outside the frame is the frame's first / last row,
	// which avirhip_band_source_rows then names, so the window holds it). No
	// frame-sized buffer: a device window is read where it lies (zero copy), a
	// host window is uploaded into a window-sized staging buffer -- and so is a
	// device window that overlaps its destination band, which would otherwise be
	// read where it lies while the band is written.
	const size_t win_off = (size_t) win_first * p -> src_stride *
		dtype_size( p -> in_type );
	const bool aside = ( host || shared );
	bool native = false;

	if( getenv( "AVIRHIP_NO_NATIVE_WINDOW" ) == nullptr )
	{
		// (alignment of the pointers the kernel will see: the staging buffers
		// are 256-byte aligned, win_off is a multiple of the row pitch)
		const void* const vsrc = (const char*) ( !aside ?
			src : (const void*) (uintptr_t) 256 ) - ( win_off & 255 );
		const void* const vdst = ( dst_mem == AVIRHIP_MEM_DEVICE ? dst :
			(const void*) (uintptr_t) 256 );
		const int xpath = ( p -> path != 0 ? p -> path : p -> auto_path );

		native = ( xpath == 4 && ( p -> is_lancir ?
			lanc2_takes_window( p, vsrc, vdst ) :
			up2_takes_window( p, vsrc, vdst )));
	}

	if( native )
	{
		// (pointer arithmetic only: nothing below row win_first is ever read)
		r.stage_bytes = r.copy_bytes = ( aside ? win_bytes : 0 );
		r.base_off = win_off;
		r.win.first = win_first;
		r.win.rows = win_rows;
	}
	else
	{
		// Other plans: the window's rows go to their place in a frame-sized
		// staging buffer of the plan -- the only source bytes that move (SURVEY.md
		// 8e: "GPU g receives source rows [r0 - halo, r1 + halo]"); the kernels
		// then run as on a whole frame, and whatever they load outside the window
		// never reaches a result (avirhip_band_source_rows).
		r.stage_bytes = src_bytes;
		r.copy_bytes = win_bytes;
		r.copy_at = win_off;
	}

	return( r );
}

// the source copy of a route, if it has one
static hipError_t copy_source( avirhip_plan* p, const SrcRoute& r,
	const void* src, hipStream_t st )
{
	return( r.copy_bytes == 0 ? hipSuccess : hipMemcpyAsync(
		(char*) p -> stage_src + r.copy_at, src, r.copy_bytes, r.kind, st ));
}

// Performs a route up to the pointer the kernels read, `*dsrc`: grows the
// staging buffer, issues the copy unless it is a late one.
static int stage_source( avirhip_plan* p, const SrcRoute& r, const void* src,
	hipStream_t st, const void** dsrc )
{
	const int rc = grow( p, &p -> stage_src, &p -> stage_src_bytes,
		r.stage_bytes );
	if( rc != 0 ) return( rc );

	if( !r.late )
	{
		AVIRHIP_HIPCHECK( copy_source( p, r, src, st ));
	}

	*dsrc = (const void*) ( (uintptr_t) ( r.stage_bytes != 0 ?
		p -> stage_src : src ) - r.base_off );
	return( AVIRHIP_OK );
}

// `win_rows` > 0: `src` holds only the source rows [win_first, win_first +
// win_rows) of the frame (avirhip_resize_window); otherwise the whole frame.
static int exec_any( avirhip_plan* p, const void* src, int src_mem, void* dst,
	int dst_mem, int row0, int row1, void* stream, int win_first = 0,
	int win_rows = 0 )
{
	src_mem = avirhip_resolve_mem( src, src_mem );
	dst_mem = avirhip_resolve_mem( dst, dst_mem );
	bool nothing;
	int rc = check_call( p, src, dst, row0, row1, win_first, win_rows, nothing );

	if( rc != 0 || nothing )
	{
		return( rc );
	}

	hipStream_t st = (hipStream_t) stream;
	DeviceGuard devguard( p -> device );
	const bool windowed = ( win_rows > 0 );
	const bool host_src = ( src_mem == AVIRHIP_MEM_HOST );
	const bool host_dst = ( dst_mem == AVIRHIP_MEM_HOST );
	const size_t src_bytes = image_bytes( p -> src_h, p -> src_stride,
		p -> src_w, p -> io_ch, p -> in_type );
	const size_t row_bytes = (size_t) p -> new_stride *
		dtype_size( p -> out_type );
	const size_t payload = (size_t) p -> new_w * p -> io_ch *
		dtype_size( p -> out_type );
	const size_t dst_bytes = ( row1 > row0 ?
		(size_t) ( row1 - row0 - 1 ) * row_bytes + payload : 0 );
	// (NewBuf may alias SrcBuf, avir.h:4650-4652)
	const bool alias = ( !windowed &&
		share_bytes( src, src_bytes, dst, dst_bytes ));

	// Calls on one plan share its scratch buffers: serialise them (the
	// reference allows concurrent resizeImage() calls on one object). The
	// only scratch-free case, device-resident float RGBA through the
	// single-launch 2x kernel, skips this -- when that kernel cannot refuse the
	// call and fall back to the generic kernels (which use scratch).
	// (CLancIR is not thread-safe in the reference either, lancir.h:319-349:
	// its plans always take the lock, and may allocate scratch under it)
	const bool scratch_free = ( !p -> is_lancir && !windowed && !alias &&
		( p -> path != 0 ? p -> path : p -> auto_path ) == 4 &&
		src_mem == AVIRHIP_MEM_DEVICE && dst_mem == AVIRHIP_MEM_DEVICE &&
		// (stricter than the kernel, which stores 8-byte pieces: kept, so that
		// no call moves between the locked and the lock-free route)
		( (uintptr_t) dst & 15 ) == 0 &&
		up2_takes_window( p, src, dst ));

	std::unique_lock< std::mutex > held;
	avirhip_plan* const q = ( scratch_free ? p : scratch_owner( p, held ));
	PerThreadRecord ptrec = { q, st, false };

	if( !scratch_free )
	{
		rc = order_behind_last_call( q, st, ptrec.on );
		if( rc != 0 ) return( rc );
	}

	const SrcRoute route = src_route( q, src, src_mem, dst, dst_mem, row0, row1,
		win_first, win_rows );
	const void* dsrc;
	void* ddst = dst;

	rc = stage_source( q, route, src, st, &dsrc );
	if( rc != 0 ) return( rc );

	if( host_dst )
	{
		rc = grow( q, &q -> stage_dst, &q -> stage_dst_bytes, dst_bytes );
		if( rc != 0 ) return( rc );

		ddst = q -> stage_dst;
	}

	// (an aliasing call: result rows copied down while source rows still travel
	// up would overwrite them -- such calls keep the serial order, whole source
	// up first)
	if( host_src && host_dst && !windowed && !alias && row0 == 0 &&
		row1 == q -> new_h && payload == row_bytes )
	{
		rc = exec_host_pipelined( q, src, dst, src_bytes, dst_bytes, row_bytes,
			st );

		if( rc != 1 )
		{
			return( rc );
		}
	}

	if( route.late )
	{
		AVIRHIP_HIPCHECK( copy_source( q, route, src, st ));
	}

	rc = exec_device( q, dsrc, ddst, row0, row1, st, route.win );
	if( rc != 0 ) return( rc );

	if( host_dst )
	{
		if( payload == row_bytes || row1 - row0 < 2 )
		{
			AVIRHIP_HIPCHECK( hipMemcpyAsync( dst, ddst, dst_bytes,
				hipMemcpyDeviceToHost, st ));
		}
		else
		{
			// padded destination rows (CLancIRParams::NewSSize): the bytes
			// between rows belong to the caller
			AVIRHIP_HIPCHECK( hipMemcpy2DAsync( dst, row_bytes, ddst,
				row_bytes, payload, (size_t) ( row1 - row0 ),
				hipMemcpyDeviceToHost, st ));
		}

		AVIRHIP_HIPCHECK( hipStreamSynchronize( st ));
	}
	else
	if( host_src )
	{
		AVIRHIP_HIPCHECK( hipStreamSynchronize( st ));
	}

	return( AVIRHIP_OK );
}

size_t plan_device_bytes( avirhip_plan* p )
{
	if( p == nullptr )
	{
		return( 0 );
	}

	size_t b = p -> alloc_bytes + plan_device_bytes( p -> inner );

	{
		std::lock_guard< std::mutex > sl( p -> spare_mtx );

		for( size_t i = 0; i < p -> spares.size(); i++ )
		{
			b += plan_device_bytes( p -> spares[ i ]);
		}
	}

	// (replicas are only touched under shard_mtx, which a sharded call holds
	// for its whole duration: do not wait for it, count what can be seen)
	if( p -> shard_mtx.try_lock())
	{
		for( size_t i = 0; i < p -> replicas.size(); i++ )
		{
			b += plan_device_bytes( p -> replicas[ i ]);
		}

		p -> shard_mtx.unlock();
	}

	return( b );
}

static avirhip_plan* new_plan()
{
	avirhip_plan* p = new avirhip_plan();
	p -> is_lancir = 0; p -> device = 0; p -> alloc_bytes = 0;
	p -> path = 0; p -> variant = 0; p -> fused_ok = 0; p -> auto_path = 1; p -> fused = nullptr; p -> tile64 = nullptr; p -> up2 = nullptr; p -> lanc2 = nullptr; p -> gpass = nullptr;
	p -> avirp.store( nullptr );
	p -> packed = nullptr; p -> resbuf = nullptr; p -> lres = nullptr;
	p -> stage_src = nullptr; p -> stage_dst = nullptr;
	p -> stage_src_bytes = 0; p -> stage_dst_bytes = 0;
	p -> shard_band = nullptr; p -> shard_band_bytes = 0; p -> shard_ldev = -1;
	p -> last_done = nullptr; p -> last_stream = nullptr; p -> last_used = false;
	p -> last_recorded = false;
	p -> pipe_in = nullptr; p -> pipe_out = nullptr;
	p -> shard_src = nullptr; p -> shard_src_bytes = 0;
	p -> tr_mul = 1.0; p -> pk_out = 0.0;
	p -> gamma = 0; p -> alpha_index = -1; p -> d_srgb_tbl = nullptr;
	p -> d_gthr = nullptr;
	p -> dither = AVIRHIP_DITHER_DEF; p -> fp4 = 0; p -> errd_line = nullptr;
	p -> is_spare = 0;
	p -> ch = 0; p -> io_ch = 0;
	p -> l_out_mul = 1.0f; p -> l_clamp = 0.0f; p -> l_unity = 1;
	p -> inner = nullptr; p -> l_order = 4;
	(void) hipGetDevice( &p -> device );
	return( p );
}

} // namespace avirhip

using namespace avirhip;

extern "C" {

int avirhip_device_count( void )
{
	int n = 0;

	if( hipGetDeviceCount( &n ) != hipSuccess )
	{
		return( 0 );
	}

	int good = 0;

	for( int i = 0; i < n; i++ )
	{
		hipDeviceProp_t pr;

		if( hipGetDeviceProperties( &pr, i ) == hipSuccess &&
			strncmp( pr.gcnArchName, "gfx950", 6 ) == 0 )
		{
			good++;
		}
	}

	return( good );
}

int avirhip_init( int device )
try
{
	avirhip::clear_error();
	if( avirhip_device_count() < 1 )
	{
		set_error( "no gfx950 device visible" );
		return( AVIRHIP_ENODEV );
	}

	AVIRHIP_HIPCHECK( hipSetDevice( device ));
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_init )

const char* avirhip_last_error( void )
{
	return( g_err );
}

const char* avirhip_version( void )
{
	return( "avirhip 0.2 (gfx950; avir v3.1 hot path; float16 images)" );
}

int avirhip_plan_create( const avirhip_plan_desc* d, avirhip_plan** out )
try
{
	avirhip::clear_error();
	if( d == nullptr || out == nullptr )
	{
		set_error( "null argument" );
		return( AVIRHIP_EINVAL );
	}

	*out = nullptr;

	if( d -> src_w < 1 || d -> src_h < 1 || d -> new_w < 1 || d -> new_h < 1 ||
		d -> channels < 1 || d -> channels > 4 || d -> in_type < 0 ||
		d -> out_type < 0 || !avir_dtype_ok( d -> in_type ) ||
		!avir_dtype_ok( d -> out_type ))
	{
		set_error( "bad image geometry / types" );
		return( AVIRHIP_EINVAL );
	}

	// half / bfloat16 elements are defined by fpclass_def<float>'s float32
	// call alone (avirhip.h, AVIRHIP_F16 / AVIRHIP_BF16)
	if(( dtype_is_float16_kind( d -> in_type ) ||
		dtype_is_float16_kind( d -> out_type )) &&
		( d -> work_f64 || d -> dither == AVIRHIP_DITHER_DEF_RNE ))
	{
		set_error( "half / bfloat16 elements: fpclass_def<float> only (not "
			"fpclass_float4, not the double pipeline)" );
		return( AVIRHIP_EUNSUPPORTED );
	}

	if( !geometry_ok( "plan_create", d -> src_w, d -> src_h,
		d -> src_stride_elems, d -> new_w, d -> new_h, 0, d -> channels,
		d -> in_type, d -> out_type ))
	{
		return( AVIRHIP_EINVAL );
	}

	PlanHold hold( new_plan() );
	avirhip_plan* const p = hold.p;
	p -> src_w = d -> src_w; p -> src_h = d -> src_h;
	p -> src_stride = ( d -> src_stride_elems < 1 ?
		d -> src_w * d -> channels : d -> src_stride_elems );
	p -> new_w = d -> new_w; p -> new_h = d -> new_h;
	p -> new_stride = d -> new_w * d -> channels;
	p -> ch = d -> channels;
	p -> io_ch = d -> channels;
	p -> in_type = d -> in_type; p -> out_type = d -> out_type;
	p -> tr_mul = d -> tr_mul; p -> pk_out = d -> pk_out;
	p -> gamma = ( d -> use_srgb_gamma ? 1 : 0 );
	// the reference treats only AlphaIndex 0 and 3 of 4-channel pixels as an
	// alpha channel (avir.h:2859/2874, 3002/3016); any other value gamma-
	// converts all four channels
	p -> alpha_index = ( d -> channels == 4 && ( d -> alpha_index == 0 ||
		d -> alpha_index == 3 ) ? d -> alpha_index : -1 );

	if( d -> dither != AVIRHIP_DITHER_DEF && d -> dither != AVIRHIP_DITHER_ERRD &&
		d -> dither != AVIRHIP_DITHER_DEF_RNE )
	{
		set_error( "unknown ditherer %d", d -> dither );
		return( AVIRHIP_EINVAL );
	}

	// float / double output skips the dither stage (avir.h:5002-5025)
	p -> dither = ( d -> out_type == AVIRHIP_U8 || d -> out_type == AVIRHIP_U16 ?
		d -> dither : AVIRHIP_DITHER_DEF );
	// fpclass_float4 (AVIRHIP_DITHER_DEF_RNE): no in-place float output
	p -> fp4 = ( d -> dither == AVIRHIP_DITHER_DEF_RNE ? 1 : 0 );

	p -> f64 = ( d -> work_f64 ? 1 : 0 );

	if( p -> f64 && ( p -> dither != AVIRHIP_DITHER_DEF || p -> fp4 ))
	{
		set_error( "the double pipeline runs the default ditherer only" );
		return( AVIRHIP_EUNSUPPORTED );
	}

	int rc = lower_axis( d -> h, d -> src_w, d -> new_w, p -> h, p -> f64 != 0 );

	if( rc == 0 ) rc = lower_axis( d -> v, d -> src_h, d -> new_h, p -> v,
		p -> f64 != 0 );

	if( rc == 0 ) rc = finalize_avir_plan( p );

	if( rc != 0 )
	{
		return( rc );
	}

	*out = hold.release();
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_plan_create )

} // extern "C"

namespace avirhip {

// Device side of an AVIR plan whose axes are lowered (host vectors filled):
// uploads, channel padding decision, fast-path preparation -- on the current
// device. Shared by plan creation and by the per-device replicas of
// avirhip_resize_sharded.
int finalize_avir_plan( avirhip_plan* p )
{
	int rc = upload_axis( p, p -> h );
	if( rc == 0 ) rc = upload_axis( p, p -> v );

	if( rc == 0 && p -> gamma )
	{
		std::vector< float > tbl( 256 );
		srgb_u8_table( tbl.data() );
		rc = upload( p, tbl, &p -> d_srgb_tbl );

		// uint8 output: the de-linearising output stage as a threshold table
		// (generic.hip; the default ditherer only)
		if( rc == 0 && p -> out_type == AVIRHIP_U8 &&
			p -> dither == AVIRHIP_DITHER_DEF )
		{
			std::vector< float > thr( 512 );

			if( gamma_u8_thresholds( 255.0f, p -> tr_mul != 1.0,
				(float) p -> tr_mul, (float) ( 1.0 / p -> tr_mul ),
				(float) p -> pk_out, thr.data() ))
			{
				rc = upload( p, thr, &p -> d_gthr );
			}
		}
	}

	if( rc == 0 && p -> f64 )
	{
		// the double pipeline: LDS-tiled two-pass kernels in double (tile64.hip;
		// reported as path 2), or -- plans with a filtered upsample, and path 1
		// on request -- one launch per op (generic64.hip)
		rc = tile64_prepare( p );
		p -> auto_path = ( rc == 0 && tile64_ok( p ) ? 2 : 1 );
		p -> fused_ok = ( rc == 0 && tile64_ok( p ) ? 1 : 0 );
		return( rc );
	}

	// 1-3 channel pixels: channels are independent, so executing them as
	// RGBA with zero padding (written by the pack stage, dropped by the
	// epilogue) is bit-identical and opens the RGBA fast paths -- 4/3 of the
	// arithmetic on kernels several times faster than the generic ones.
	if( rc == 0 && p -> io_ch < 4 )
	{
		p -> ch = 4;
	}

	if( rc == 0 ) rc = fused_prepare( p );
	if( rc == 0 ) rc = up2_prepare( p );
	if( rc == 0 ) rc = gpass_prepare( p );

	if( rc == 0 && gpass_ok( p ))
	{
		p -> fused_ok |= 8;

		// exact 2x keeps its marching kernel; otherwise the pass kernels
		// where they measured faster than the tiles (gpass_preferred)
		if( p -> auto_path != 4 && !fused_dn_both( p ) &&
			gpass_preferred( p ))
		{
			p -> auto_path = 5;
		}

		// exact 2x with integer pixels on both sides: the pass kernels read
		// and write the caller's images themselves, the marching kernel
		// needs a pack pass before and an epilogue pass behind it
		// (1920x1080 -> 3840x2160 RGB u8: 0.084 against 0.089 ms)
		// ... in general: whenever the marching kernel's result needs the
		// epilogue pass (integer or 1-3 channel pixels out; 1080p -> 4K:
		// RGB float 0.071 against 0.101 ms, RGB u8 -> float 0.070 / 0.102,
		// RGBA float -> u8 0.082 / 0.087); RGBA float output keeps it (a
		// uint8 RGBA source costs it one pack pass: 0.064 against 0.068)
		// Round 4: the marching kernel's vertical phase stores uint8 / uint16
		// / narrow float pixels itself (up2_stores_io): no epilogue, and from
		// 1080p sources on it is ahead of the pass kernels again (tools/
		// up2_io_sweep.py: 1920x1080 RGB u8 0.063 against 0.080 ms, u16 0.062 /
		// 0.102, RGBA float -> u8 0.053 / 0.084; 3840x2160 RGB u8 0.154 / 0.314;
		// 1280x720 RGB u8 0.046 / 0.044: the pass kernels keep small frames)
		const bool up2_io = ( p -> auto_path == 4 && up2_stores_io( p ) &&
			(long) p -> src_w * p -> src_h >= 1500000L );

		if( p -> auto_path == 4 && gpass_preferred( p ) && !p -> gamma &&
			!up2_io && p -> dither == AVIRHIP_DITHER_DEF &&
			!( p -> out_type == AVIRHIP_F32 && p -> io_ch == 4 ) &&
			( p -> out_type == AVIRHIP_U8 || p -> out_type == AVIRHIP_U16 ||
			p -> out_type == AVIRHIP_F32 ))
		{
			p -> auto_path = 5;
		}
	}

	if( rc == 0 && p -> ch != p -> io_ch && p -> auto_path == 1 )
	{
		// no fast path for this plan: run the generic kernels unpadded
		fused_release( p );
		tile64_release( p );
		up2_release( p );
		gpass_release( p );
		p -> ch = p -> io_ch;
		p -> fused_ok = 0;
	}

	return( rc );
}

static int finalize_lancir_plan( avirhip_plan* p )
{
	int rc = AVIRHIP_OK;
	LancirAxisDev* ax[ 2 ] = { &p -> lv, &p -> lh };

	for( int i = 0; i < 2 && rc == 0; i++ )
	{
		LancirAxisDev& L = *ax[ i ];
		if( rc == 0 ) rc = upload( p, L.h_flt, &L.d_flt );
		if( rc == 0 ) rc = upload( p, L.h_start, &L.d_start );
		if( rc == 0 ) rc = upload( p, L.h_fidx, &L.d_fidx );
	}

	if( rc == 0 ) rc = fused_prepare( p );
	if( rc == 0 ) rc = lanc2_prepare( p );
	if( rc == 0 ) rc = gpass_prepare( p );

	if( rc == 0 && gpass_ok( p ))
	{
		p -> fused_ok |= 8;

		// exact 2x: the marching kernel from 1080p sources on; smaller frames
		// take the pass kernels / the fused k_lf (tools/lanc2_io_sweep.py:
		// 640x480 float RGBA 0.012 against 0.023 ms, 1280x720 0.022 / 0.027,
		// 1920x1080 0.042 / 0.035; RGB uint8 0.043 / 0.050 at 720p, 0.072 /
		// 0.062 at 1080p, 0.255 / 0.140 at 2160p)
		if( p -> auto_path != 4 ||
			(long) p -> src_w * p -> src_h < 1500000L )
		{
			p -> auto_path = 5;
		}
	}

	// RGBA with integer elements or an output gain: the fast kernels compute
	// in float RGBA with unity gain -- run them in an inner plan of that
	// kind, between the pack pass and the output stage (both of which are
	// what the reference does around its float core, lancir.h:541-710)
	if( rc == 0 && p -> auto_path == 1 && p -> inner == nullptr &&
		!( p -> io_ch == 4 && p -> in_type == AVIRHIP_F32 &&
		p -> out_type == AVIRHIP_F32 && p -> l_unity ) &&
		getenv( "AVIRHIP_NO_INNER" ) == nullptr )
	{
		PlanHold qhold( new_plan() );
		avirhip_plan* const q = qhold.p;
		q -> device = p -> device;
		q -> is_lancir = 1;
		q -> src_w = p -> src_w; q -> src_h = p -> src_h;
		q -> src_stride = p -> src_w * 4;
		q -> new_w = p -> new_w; q -> new_h = p -> new_h;
		q -> new_stride = p -> new_w * 4;
		q -> ch = 4; q -> io_ch = 4;
		q -> in_type = AVIRHIP_F32; q -> out_type = AVIRHIP_F32;
		q -> lv = p -> lv; q -> lh = p -> lh; // (device pointers re-uploaded)
		// 1-3 channels run zero-padded to RGBA, in THEIR summation order
		q -> l_order = p -> io_ch;
		rc = finalize_lancir_plan( q );

		if( rc == 0 && q -> auto_path != 1 )
		{
			p -> inner = qhold.release();
			p -> auto_path = q -> auto_path;
			p -> fused_ok |= ( q -> fused_ok & ( 4 | 8 ));
		}
	}

	return( rc );
}

// A replica of plan `s` on device `device` (same tables, its own uploads,
// scratch and fast-path state).
static int clone_plan( const avirhip_plan* s, int device, avirhip_plan** out )
{
	AVIRHIP_HIPCHECK( hipSetDevice( device ));
	PlanHold hold( new_plan() );
	avirhip_plan* const q = hold.p;
	q -> is_lancir = s -> is_lancir;
	q -> src_w = s -> src_w; q -> src_h = s -> src_h;
	q -> src_stride = s -> src_stride;
	q -> new_w = s -> new_w; q -> new_h = s -> new_h;
	q -> new_stride = s -> new_stride;
	q -> ch = s -> io_ch; q -> io_ch = s -> io_ch;
	q -> in_type = s -> in_type; q -> out_type = s -> out_type;
	q -> tr_mul = s -> tr_mul; q -> pk_out = s -> pk_out;
	q -> gamma = s -> gamma; q -> alpha_index = s -> alpha_index;
	q -> dither = s -> dither;
	q -> fp4 = s -> fp4;
	q -> f64 = s -> f64;
	q -> l_out_mul = s -> l_out_mul; q -> l_clamp = s -> l_clamp;
	q -> l_unity = s -> l_unity;
	q -> l_order = s -> l_order;
	q -> h = s -> h; q -> v = s -> v;     // host vectors; device pointers are
	q -> lv = s -> lv; q -> lh = s -> lh; // replaced by the uploads below
	q -> path = s -> path;
	q -> variant = s -> variant;

	const int rc = ( s -> is_lancir ? finalize_lancir_plan( q ) :
		finalize_avir_plan( q ));

	if( rc != 0 )
	{
		return( rc );
	}

	if( q -> inner != nullptr )
	{
		q -> inner -> path = q -> path;
		q -> inner -> variant = q -> variant;
	}

	*out = hold.release();
	return( AVIRHIP_OK );
}

// The forced path and variant of a plan hold for everything that runs its
// calls: its inner plan, its same-device spares and other-device replicas, and
// their inner plans. They are pushed when they are set (and copied by
// clone_plan), never per call.
static void push_forced( avirhip_plan* p )
{
	const int path = p -> path;
	const int variant = p -> variant;
	auto set = [ path, variant ]( avirhip_plan* q )
	{
		for( ; q != nullptr; q = q -> inner )
		{
			q -> path = path;
			q -> variant = variant;
		}
	};

	set( p -> inner );
	{
		std::lock_guard< std::mutex > sl( p -> spare_mtx );

		for( size_t i = 0; i < p -> spares.size(); i++ )
		{
			set( p -> spares[ i ]);
		}
	}
	{
		std::lock_guard< std::mutex > sl( p -> shard_mtx );

		for( size_t i = 0; i < p -> replicas.size(); i++ )
		{
			set( p -> replicas[ i ]);
		}
	}
}

} // namespace avirhip

extern "C" {

/* one frame, contiguous output-row bands, one band per
 * entry of `devices`, stitched into `dst`. Bands are computed with global
 * indices, so the stitched frame is bit-identical to avirhip_resize(). */
int avirhip_resize_sharded( avirhip_plan* p, int n_gpus, const int* devices,
	const void* src, void* dst, int gather_root, double* t_compute_ms,
	double* t_gather_ms )
try
{
	avirhip::clear_error();
	if( p == nullptr || n_gpus < 1 || src == nullptr || dst == nullptr ||
		( devices == nullptr && n_gpus > 1 ) || gather_root < 0 ||
		gather_root >= n_gpus )
	{
		set_error( "resize_sharded: bad arguments" );
		return( AVIRHIP_EINVAL );
	}

	int ndev = 0;
	AVIRHIP_HIPCHECK( hipGetDeviceCount( &ndev ));
	const int src_mem = avirhip_resolve_mem( src, AVIRHIP_MEM_AUTO );
	const int dst_mem = avirhip_resolve_mem( dst, AVIRHIP_MEM_AUTO );
	int src_dev = -1;

	if( src_mem == AVIRHIP_MEM_DEVICE )
	{
		hipPointerAttribute_t at;
		AVIRHIP_HIPCHECK( hipPointerGetAttributes( &at, src ));
		src_dev = at.device;
	}

	int dst_dev = -1;

	if( dst_mem == AVIRHIP_MEM_DEVICE )
	{
		hipPointerAttribute_t at;
		AVIRHIP_HIPCHECK( hipPointerGetAttributes( &at, dst ));
		dst_dev = at.device;
	}

	const bool force_replica =
		( getenv( "AVIRHIP_SHARDED_FORCE_REPLICA" ) != nullptr );
	// test aid: AVIRHIP_SHARDED_DEVMAP="0,0,0" maps the LOGICAL devices of
	// `devices[]` (0, 1, 2) onto physical ones, so that the multi-device
	// branches -- one replica and one set of buffers per logical device, the
	// source copied to each, stores / copies into a peer's memory at the
	// band's offset -- execute on a box with a single GPU
	std::vector< int > devmap;
	{
		const char* dm = getenv( "AVIRHIP_SHARDED_DEVMAP" );

		while( dm != nullptr && *dm != 0 )
		{
			devmap.push_back( atoi( dm ));
			dm = strchr( dm, ',' );
			if( dm != nullptr ) dm++;
		}
	}

	const bool mocked = !devmap.empty();
	// test aid: always go through the band buffers + peer copies
	const bool force_staged =
		( getenv( "AVIRHIP_SHARDED_STAGED" ) != nullptr );

	const size_t esz_out = dtype_size( p -> out_type );
	const size_t src_bytes = image_bytes( p -> src_h, p -> src_stride,
		p -> src_w, p -> io_ch, p -> in_type );
	const size_t row_bytes = (size_t) p -> new_stride * esz_out;

	// the replica list and the per-replica band / source buffers are shared
	// by every sharded call on this plan; the caller's current device comes
	// back on every way out
	std::lock_guard< std::mutex > shard_lock( p -> shard_mtx );
	DeviceGuard devkeep;
	std::vector< avirhip_plan* > pl( n_gpus );
	std::vector< int > r0( n_gpus ), r1( n_gpus );
	std::vector< char* > band( n_gpus );
	int rc = AVIRHIP_OK;
	const auto t0 = std::chrono::steady_clock::now();

	// ---- compute: every band on its device's default stream
	for( int g = 0; g < n_gpus && rc == 0; g++ )
	{
		// ld: the device as the caller names it; d: where it really is
		const int ld = ( devices != nullptr ? devices[ g ] : p -> device );
		const int d = ( mocked && ld >= 0 && ld < (int) devmap.size() ?
			devmap[ ld ] : ld );

		if( d < 0 || d >= ndev || ld < 0 )
		{
			set_error( "resize_sharded: device %d does not exist", ld );
			rc = AVIRHIP_EINVAL;
			break;
		}

		avirhip_plan* q = nullptr;

		if( ld == p -> device && !force_replica )
		{
			q = p;
		}
		else
		{
			for( size_t i = 0; i < p -> replicas.size(); i++ )
			{
				if( p -> replicas[ i ] -> shard_ldev == ld )
				{
					q = p -> replicas[ i ];
				}
			}

			if( q == nullptr )
			{
				if(( rc = clone_plan( p, d, &q )) != 0 ) break;
				q -> shard_ldev = ld;
				p -> replicas.push_back( q );
			}
		}

		pl[ g ] = q;
		r0[ g ] = (int) ( (long) p -> new_h * g / n_gpus );
		r1[ g ] = (int) ( (long) p -> new_h * ( g + 1 ) / n_gpus );
		AVIRHIP_HIPCHECK( hipSetDevice( d ));

		// the source where this device can read it
		const void* s = src;
		int smem = src_mem;

		// (mocked: the buffers live on logical device 0)
		if( src_mem == AVIRHIP_MEM_DEVICE && ( mocked ? ld != 0 : src_dev != d ))
		{
			if(( rc = grow( q, &q -> shard_src, &q -> shard_src_bytes,
				src_bytes )) != 0 ) break;

			AVIRHIP_HIPCHECK( hipMemcpyPeerAsync( q -> shard_src, d, src,
				src_dev, src_bytes, nullptr ));
			s = q -> shard_src;
		}

		// A device destination the band's device can address (its own memory,
		// or a peer's over xGMI): the kernels store the band straight into
		// `dst` -- the transfer rides under the compute, there is no gather
		// phase and no second pass over the band.
		bool direct = false;

		if( dst_mem == AVIRHIP_MEM_DEVICE && !force_staged )
		{
			if( mocked ? ld == 0 : d == dst_dev )
			{
				direct = true;
			}
			else
			if( mocked )
			{
				direct = true; // "peer" memory on the same physical device
			}
			else
			{
				int can = 0;

				if( hipDeviceCanAccessPeer( &can, d, dst_dev ) == hipSuccess &&
					can )
				{
					const hipError_t pe = hipDeviceEnablePeerAccess( dst_dev, 0 );
					direct = ( pe == hipSuccess ||
						pe == hipErrorPeerAccessAlreadyEnabled );
				}

				(void) hipGetLastError();
			}
		}

		if( direct )
		{
			band[ g ] = nullptr; // nothing to gather
			rc = exec_any( q, s, smem, (char*) dst + (size_t) r0[ g ] *
				row_bytes, AVIRHIP_MEM_DEVICE, r0[ g ], r1[ g ], nullptr );

			continue;
		}

		// bands that share a device (and plan) lie one after another in that
		// plan's band buffer: room for the whole frame covers every split
		if(( rc = grow( q, &q -> shard_band, &q -> shard_band_bytes,
			(size_t) p -> new_h * row_bytes + 16 )) != 0 ) break;

		band[ g ] = (char*) q -> shard_band + (size_t) r0[ g ] * row_bytes;
		rc = exec_any( q, s, smem, band[ g ], AVIRHIP_MEM_DEVICE, r0[ g ],
			r1[ g ], nullptr );
	}

	for( int g = 0; g < n_gpus && rc == 0; g++ )
	{
		AVIRHIP_HIPCHECK( hipSetDevice( pl[ g ] -> device ));
		AVIRHIP_HIPCHECK( hipStreamSynchronize( nullptr ));
	}

	const auto t1 = std::chrono::steady_clock::now();

	// ---- gather: band buffers -> dst (peer copies over xGMI, or D2H) for
	// the bands that could not be stored directly

	for( int g = 0; g < n_gpus && rc == 0; g++ )
	{
		const size_t bb = (size_t) ( r1[ g ] - r0[ g ]) * row_bytes;
		char* to = (char*) dst + (size_t) r0[ g ] * row_bytes;
		AVIRHIP_HIPCHECK( hipSetDevice( pl[ g ] -> device ));

		if( bb == 0 || band[ g ] == nullptr )
		{
			continue;
		}

		if( dst_mem == AVIRHIP_MEM_DEVICE )
		{
			AVIRHIP_HIPCHECK( hipMemcpyPeerAsync( to, dst_dev, band[ g ],
				pl[ g ] -> device, bb, nullptr ));
		}
		else
		{
			AVIRHIP_HIPCHECK( hipMemcpyAsync( to, band[ g ], bb,
				hipMemcpyDeviceToHost, nullptr ));
		}
	}

	for( int g = 0; g < n_gpus && rc == 0; g++ )
	{
		AVIRHIP_HIPCHECK( hipSetDevice( pl[ g ] -> device ));
		AVIRHIP_HIPCHECK( hipStreamSynchronize( nullptr ));
	}

	const auto t2 = std::chrono::steady_clock::now();

	if( t_compute_ms != nullptr )
	{
		*t_compute_ms = std::chrono::duration< double, std::milli >(
			t1 - t0 ).count();
	}

	if( t_gather_ms != nullptr )
	{
		*t_gather_ms = std::chrono::duration< double, std::milli >(
			t2 - t1 ).count();
	}

	return( rc );
}
AVIRHIP_CATCH( avirhip_resize_sharded )

static int lower_lancir_axis( avirhip_plan* p, const avirhip_lancir_axis& a,
	LancirAxisDev& L )
{
	if( a.kernel_len < 2 || ( a.kernel_len & 1 ) || a.n_filters < 1 ||
		a.filters == nullptr || a.pos == nullptr || a.dst_len < 1 ||
		a.src_len < 1 )
	{
		set_error( "malformed LANCIR axis" );
		return( AVIRHIP_EINVAL );
	}

	L.kernel_len = a.kernel_len; L.src_len = a.src_len;
	L.dst_len = a.dst_len; L.n_filters = a.n_filters;
	L.h_flt.assign( a.filters, a.filters + (size_t) a.n_filters *
		a.kernel_len );
	L.h_start.resize( a.dst_len );
	L.h_fidx.resize( a.dst_len );

	for( int j = 0; j < a.dst_len; j++ )
	{
		if( a.pos[ j ].flt_index < 0 || a.pos[ j ].flt_index >= a.n_filters )
		{
			set_error( "bad LANCIR pos[%d]", j );
			return( AVIRHIP_EINVAL );
		}

		// `so` is relative to the padded scanline; edge replication of the
		// padding (lancir.h:1541-1594, 1698-1734) becomes an index clamp.
		L.h_start[ j ] = a.pos[ j ].so - a.padl;
		L.h_fidx[ j ] = a.pos[ j ].flt_index;
	}

	return( AVIRHIP_OK );
}

int avirhip_lancir_plan_create( const avirhip_lancir_desc* d,
	avirhip_plan** out )
try
{
	avirhip::clear_error();
	if( d == nullptr || out == nullptr )
	{
		set_error( "null argument" );
		return( AVIRHIP_EINVAL );
	}

	*out = nullptr;

	if( d -> src_w < 1 || d -> src_h < 1 || d -> new_w < 1 || d -> new_h < 1 ||
		d -> channels < 1 || d -> channels > 4 )
	{
		set_error( "bad image geometry" );
		return( AVIRHIP_EINVAL );
	}

	if( d -> in_type < 0 || d -> in_type > AVIRHIP_BF16 || d -> out_type < 0 ||
		d -> out_type > AVIRHIP_BF16 )
	{
		set_error( "LANCIR: element types are uint8, uint16, uint32 (as "
			"uint16), float or double (lancir.h:373-381)" );
		return( AVIRHIP_EINVAL );
	}

	if( !geometry_ok( "lancir_plan_create", d -> src_w, d -> src_h,
		d -> src_stride_elems, d -> new_w, d -> new_h, d -> new_stride_elems,
		d -> channels, d -> in_type, d -> out_type ))
	{
		return( AVIRHIP_EINVAL );
	}

	PlanHold hold( new_plan() );
	avirhip_plan* const p = hold.p;
	p -> is_lancir = 1;
	p -> src_w = d -> src_w; p -> src_h = d -> src_h;
	p -> src_stride = ( d -> src_stride_elems < 1 ?
		d -> src_w * d -> channels : d -> src_stride_elems );
	p -> new_w = d -> new_w; p -> new_h = d -> new_h;
	p -> new_stride = ( d -> new_stride_elems < 1 ?
		d -> new_w * d -> channels : d -> new_stride_elems );
	p -> ch = d -> channels;
	p -> io_ch = d -> channels;
	p -> in_type = d -> in_type; p -> out_type = d -> out_type;
	p -> l_out_mul = d -> out_mul; p -> l_clamp = d -> clamp;
	p -> l_unity = d -> is_unity_mul;

	int rc = lower_lancir_axis( p, d -> v, p -> lv );
	if( rc == 0 ) rc = lower_lancir_axis( p, d -> h, p -> lh );
	if( rc == 0 ) rc = finalize_lancir_plan( p );

	if( rc != 0 )
	{
		return( rc );
	}

	*out = hold.release();
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_lancir_plan_create )

void avirhip_plan_destroy( avirhip_plan* p )
{
	if( p == nullptr )
	{
		return;
	}

	for( size_t i = 0; i < p -> replicas.size(); i++ )
	{
		avirhip_plan_destroy( p -> replicas[ i ]);
	}

	p -> replicas.clear();

	for( size_t i = 0; i < p -> spares.size(); i++ )
	{
		avirhip_plan_destroy( p -> spares[ i ]);
	}

	p -> spares.clear();

	if( p -> last_done != nullptr )
	{
		(void) hipEventDestroy( p -> last_done );
	}

	for( size_t i = 0; i < p -> pipe_ev.size(); i++ )
	{
		(void) hipEventDestroy( p -> pipe_ev[ i ]);
	}

	p -> pipe_ev.clear();

	if( p -> pipe_in != nullptr )
	{
		(void) hipStreamDestroy( (hipStream_t) p -> pipe_in );
		(void) hipStreamDestroy( (hipStream_t) p -> pipe_out );
	}

	avirhip_plan_destroy( p -> inner );
	p -> inner = nullptr;
	fused_release( p );
	tile64_release( p );
	up2_release( p );
	lanc2_release( p );
	gpass_release( p );
	avirp_release( p );

	for( size_t i = 0; i < p -> allocs.size(); i++ )
	{
		(void) hipFree( p -> allocs[ i ]);
	}

	delete p;
}

int avirhip_plan_set_path( avirhip_plan* p, int path )
try
{
	avirhip::clear_error();
	if( p == nullptr || path < 0 || path > 5 )
	{
		set_error( "bad path" );
		return( AVIRHIP_EINVAL );
	}

	if(( path == 2 && !( p -> fused_ok & 1 )) ||
		( path == 3 && !( p -> fused_ok & 2 )) ||
		( path == 4 && !( p -> fused_ok & 4 )) ||
		( path == 5 && !( p -> fused_ok & 8 )) ||
		( p -> is_lancir && ( path == 2 || path == 3 )))
	{
		set_error( "path %d cannot run this plan", path );
		return( AVIRHIP_EUNSUPPORTED );
	}

	p -> path = path;
	push_forced( p );
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_plan_set_path )

unsigned long long avirhip_plan_device_bytes( avirhip_plan* p )
{
	return( (unsigned long long) plan_device_bytes( p ));
}

int avirhip_plan_set_variant( avirhip_plan* p, int variant )
try
{
	avirhip::clear_error();
	if( p == nullptr || variant < 0 || variant > 255 )
	{
		set_error( "bad variant" );
		return( AVIRHIP_EINVAL );
	}

	p -> variant = variant;
	push_forced( p );
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_plan_set_variant )

int avirhip_band_source_rows( const avirhip_plan* p, int row0, int row1,
	int* first, int* last )
try
{
	avirhip::clear_error();
	if( p == nullptr || first == nullptr || last == nullptr || row0 < 0 ||
		row1 > p -> new_h || row1 <= row0 )
	{
		set_error( "band_source_rows: bad arguments" );
		return( AVIRHIP_EINVAL );
	}

	band_src_rows( p, row0, row1, first, last );
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_band_source_rows )

int avirhip_plan_get_path( const avirhip_plan* p )
try
{
	avirhip::clear_error();
	if( p == nullptr )
	{
		return( AVIRHIP_EINVAL );
	}

	return( p -> path != 0 ? p -> path : p -> auto_path );
}
AVIRHIP_CATCH( avirhip_plan_get_path )

int avirhip_resize( avirhip_plan* p, const void* src, int src_mem, void* dst,
	int dst_mem, void* stream )
try
{
	avirhip::clear_error();
	if( p == nullptr )
	{
		set_error( "null plan" );
		return( AVIRHIP_EINVAL );
	}

	return( exec_any( p, src, src_mem, dst, dst_mem, 0, p -> new_h, stream ));
}
AVIRHIP_CATCH( avirhip_resize )

int avirhip_resize_band( avirhip_plan* p, const void* src, int src_mem,
	void* dst_band, int dst_mem, int row0, int row1, void* stream )
try
{
	avirhip::clear_error();
	return( exec_any( p, src, src_mem, dst_band, dst_mem, row0, row1,
		stream ));
}
AVIRHIP_CATCH( avirhip_resize_band )

int avirhip_resize_window( avirhip_plan* p, const void* src_rows, int src_mem,
	int first_row, int n_rows, void* dst_band, int dst_mem, int row0, int row1,
	void* stream )
try
{
	avirhip::clear_error();
	if( p == nullptr || n_rows < 1 )
	{
		set_error( "resize_window: bad arguments" );
		return( AVIRHIP_EINVAL );
	}

	return( exec_any( p, src_rows, src_mem, dst_band, dst_mem, row0, row1,
		stream, first_row, n_rows ));
}
AVIRHIP_CATCH( avirhip_resize_window )

int avirhip_time_resize( avirhip_plan* p, const void* src, void* dst,
	int iters, void* stream, double* avg_ms )
try
{
	avirhip::clear_error();
	if( p == nullptr || iters < 1 || avg_ms == nullptr )
	{
		set_error( "bad arguments" );
		return( AVIRHIP_EINVAL );
	}

	hipStream_t st = (hipStream_t) stream;
	// (destroyed on every way out)
	struct Events
	{
		hipEvent_t e0, e1;
		~Events()
		{
			if( e0 != nullptr ) (void) hipEventDestroy( e0 );
			if( e1 != nullptr ) (void) hipEventDestroy( e1 );
		}
	} ev = { nullptr, nullptr };
	hipEvent_t& e0 = ev.e0, & e1 = ev.e1;
	AVIRHIP_HIPCHECK( hipEventCreate( &e0 ));
	AVIRHIP_HIPCHECK( hipEventCreate( &e1 ));
	AVIRHIP_HIPCHECK( hipEventRecord( e0, st ));

	for( int i = 0; i < iters; i++ )
	{
		int rc = exec_any( p, src, AVIRHIP_MEM_DEVICE, dst,
			AVIRHIP_MEM_DEVICE, 0, p -> new_h, stream );

		if( rc != 0 )
		{
			return( rc );
		}
	}

	AVIRHIP_HIPCHECK( hipEventRecord( e1, st ));
	AVIRHIP_HIPCHECK( hipEventSynchronize( e1 ));
	float ms = 0.0f;
	AVIRHIP_HIPCHECK( hipEventElapsedTime( &ms, e0, e1 ));
	*avg_ms = (double) ms / iters;
	return( AVIRHIP_OK );
}
AVIRHIP_CATCH( avirhip_time_resize )

} // extern "C"
