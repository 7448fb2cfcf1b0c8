// pviews.hip -- plane views of the planar calls (include/avirhip.h, "Plane
// views"): the way of a call's table of planes to the device, and the strided
// <-> tight copy of one plane that the per-plane road of a declined call runs
// around the plan's own road.
//
// The table. k_lancp / k_avirp read one PlaneViewDev (48 bytes) per workgroup,
// by plane. A call's table cannot travel as kernel arguments (a 64 x 3 batch
// is 9 KB), must not be read from the caller's array once the call has
// returned, and must not live in the plan (calls on one plan run concurrently,
// without a lock). So a call takes a SLOT of a process-wide pool: a pinned
// host buffer, a device buffer and an event. The table is copied into the
// pinned buffer by the calling thread, from there to the device buffer by a
// copy on the call's stream, and the event is recorded behind the launch; the
// slot is handed out again only when its event has passed, so neither buffer
// is overwritten while the device may still read it. The pool's mutex is held
// while a slot is looked for, never across a device call that waits. Slots are
// never freed: the pool grows to the number of calls in flight at once (per
// device and size class) and stays there.
//
// The copy. One lane an element, rows along blockIdx.y; plain loads and stores
// of the element's own width, so that a scatter into an interleaved image
// touches the plane's elements alone.

#include "plan.h"
#include <string.h>

namespace avirhip {

namespace {

struct PvSlot
{
	int device;
	size_t cap;
	void* host;
	void* devp;
	hipEvent_t ev;
	bool busy;     // a call holds it (between push and done)
	bool recorded; // `ev` has been recorded at least once
};

std::mutex pv_mtx;
std::vector< PvSlot* >& pv_slots()
{
	// (never destroyed: no HIP call runs in a static destructor)
	static std::vector< PvSlot* >* const v = new std::vector< PvSlot* >();
	return( *v );
}

PvSlot* pv_take( const int device, const size_t bytes )
{
	std::lock_guard< std::mutex > lock( pv_mtx );

	for( PvSlot* const s : pv_slots() )
	{
		if( s -> busy || s -> device != device || s -> cap < bytes )
		{
			continue;
		}

		if( s -> recorded && hipEventQuery( s -> ev ) != hipSuccess )
		{
			(void) hipGetLastError(); // (hipErrorNotReady is no error)
			continue;
		}

		s -> busy = true;
		return( s );
	}

	return( nullptr );
}

template< typename T >
__global__ void __launch_bounds__( 256 ) k_pview_copy( const char* const src,
	const long s_pb, const long s_eb, char* const dst, const long d_pb,
	const long d_eb, const int w, const int h )
{
	const int c = blockIdx.x * 256 + threadIdx.x;

	if( c >= w )
	{
		return;
	}

	for( int r = blockIdx.y; r < h; r += gridDim.y )
	{
		*(T*) ( dst + (long) r * d_pb + (long) c * d_eb ) =
			*(const T*) ( src + (long) r * s_pb + (long) c * s_eb );
	}
}

} // namespace

int PlaneViewUpload :: push( const PlaneViewTable& t, const int device,
	hipStream_t st )
{
	const size_t bytes = t.size() * sizeof( PlaneViewDev );
	PvSlot* s = pv_take( device, bytes );

	if( s == nullptr )
	{
		size_t cap = 4096;

		while( cap < bytes )
		{
			cap *= 2;
		}

		s = new PvSlot();
		s -> device = device; s -> cap = cap; s -> host = nullptr;
		s -> devp = nullptr; s -> ev = nullptr; s -> busy = true;
		s -> recorded = false;
		hipError_t e = hipHostMalloc( &s -> host, cap, hipHostMallocDefault );
		if( e == hipSuccess ) e = hipMalloc( &s -> devp, cap );
		if( e == hipSuccess ) e = hipEventCreateWithFlags( &s -> ev,
			hipEventDisableTiming );

		if( e != hipSuccess )
		{
			if( s -> devp != nullptr ) (void) hipFree( s -> devp );
			if( s -> host != nullptr ) (void) hipHostFree( s -> host );
			delete s;
			AVIRHIP_HIPCHECK( e );
		}

		std::lock_guard< std::mutex > lock( pv_mtx );
		pv_slots().push_back( s );
	}

	slot = s;
	pushed = st;
	memcpy( s -> host, t.data(), bytes );
	AVIRHIP_HIPCHECK( hipMemcpyAsync( s -> devp, s -> host, bytes,
		hipMemcpyHostToDevice, st ));
	return( AVIRHIP_OK );
}

const PlaneViewDev* PlaneViewUpload :: dev() const
{
	return( (const PlaneViewDev*) ((PvSlot*) slot ) -> devp );
}

void PlaneViewUpload :: done( hipStream_t st )
{
	PvSlot* const s = (PvSlot*) slot;

	if( s == nullptr )
	{
		return;
	}

	slot = nullptr;
	const bool rec = ( hipEventRecord( s -> ev, st ) == hipSuccess );
	std::lock_guard< std::mutex > lock( pv_mtx );

	if( rec )
	{
		// (an event that could not be recorded keeps the slot out of use)
		s -> recorded = true;
		s -> busy = false;
	}
}

PlaneViewUpload :: ~PlaneViewUpload()
{
	// a call that failed between push() and done(): the copy may be in flight
	// on its stream; the slot comes back once an event behind it has passed
	done( pushed );
}

int pview_copy( const void* src, const long s_pb, const long s_eb, void* dst,
	const long d_pb, const long d_eb, const int w, const int h, const int es,
	hipStream_t st )
{
	if( w < 1 || h < 1 )
	{
		return( AVIRHIP_OK );
	}

	const dim3 grid( (unsigned) (( w + 255 ) / 256 ),
		(unsigned) ( h < 65535 ? h : 65535 ));

#define PV_GO( T ) hipLaunchKernelGGL(( k_pview_copy< T > ), grid, dim3( 256 ), \
		0, st, (const char*) src, s_pb, s_eb, (char*) dst, d_pb, d_eb, w, h )

	switch( es )
	{
		case 1: PV_GO( unsigned char ); break;
		case 2: PV_GO( unsigned short ); break;
		case 4: PV_GO( unsigned int ); break;
		case 8: PV_GO( unsigned long long ); break;
		default:
			set_error( "pview_copy: element size %d", es );
			return( AVIRHIP_EINTERNAL );
	}
#undef PV_GO

	AVIRHIP_HIPCHECK( hipGetLastError() );
	return( AVIRHIP_OK );
}

} // namespace avirhip
