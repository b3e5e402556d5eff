// The RCCL loader, the communicator (wh_comm_*) and the arena broadcast.
#include "runtime.h"

// ncclUniqueId by value, as ncclCommInitRank takes it (rccl.h: struct { char internal[128]; })
struct ncclUniqueIdBlob { char internal[ 128 ]; };

extern "C" {

// ------------------------------------------------------------------------------------------------------------------
// RCCL: the arena of rank `root` into every rank's arena (one process per GPU). librccl.so is opened on first use.
// ------------------------------------------------------------------------------------------------------------------
namespace
{
	struct RcclApi
	{
		void* lib = nullptr;
		int ( *getUniqueId )( void* ) = nullptr;
		int ( *commInitRank )( void**, int, ncclUniqueIdBlob, int ) = nullptr;
		int ( *commDestroy )( void* ) = nullptr;
		int ( *broadcast )( const void*, void*, size_t, int, int, void*, hipStream_t ) = nullptr;
		int ( *allReduce )( const void*, void*, size_t, int, int, void*, hipStream_t ) = nullptr;
		const char* ( *errorString )( int ) = nullptr;
		int ( *getVersion )( int* ) = nullptr;	   // optional
		std::string why, loadedAs;
	};
	RcclApi* rccl()
	{
		static RcclApi api;
		static std::once_flag once;
		std::call_once( once, []() {
			const char* names[] = { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so" };
			for( const char* n : names )
			{
				api.lib = dlopen( n, RTLD_NOW | RTLD_LOCAL );
				if( api.lib ) { api.loadedAs = n; break; }
			}
			if( !api.lib )
			{
				const char* e = dlerror();
				api.why = std::string( "librccl.so not found: " ) + ( e ? e : "" );
				return;
			}
			auto sym = [ & ]( const char* name ) -> void* {
				void* p = dlsym( api.lib, name );
				if( !p && api.why.empty() ) api.why = std::string( "librccl.so lacks " ) + name;
				return p;
			};
			api.getUniqueId = (decltype( api.getUniqueId ))sym( "ncclGetUniqueId" );
			api.commInitRank = (decltype( api.commInitRank ))sym( "ncclCommInitRank" );
			api.commDestroy = (decltype( api.commDestroy ))sym( "ncclCommDestroy" );
			api.broadcast = (decltype( api.broadcast ))sym( "ncclBroadcast" );
			api.allReduce = (decltype( api.allReduce ))sym( "ncclAllReduce" );
			api.errorString = (decltype( api.errorString ))sym( "ncclGetErrorString" );
			api.getVersion = (decltype( api.getVersion ))dlsym( api.lib, "ncclGetVersion" );
		} );
		return &api;
	}
	int rcclFail( int rc, const char* what )
	{
		RcclApi* r = rccl();
		setError( std::string( what ) + ": " + ( r->errorString ? r->errorString( rc ) : "RCCL error" ) );
		return WH_E_HIP;
	}
}	// namespace

struct wh_comm
{
	void* comm = nullptr;
	int rank = 0, world = 1;
	hipStream_t stream = nullptr;
	int* scratch = nullptr;
	double timeout = 0.0;	   // seconds a collective may take before the call gives up (0 = wait for ever)
};

namespace
{
	// Waits for the communicator's stream like hipStreamSynchronize, but not for ever: a rank that never arrives at a collective
	// must turn into an error on the ranks that did, not into a hung node (RCCL itself has no deadline).
	int waitComm( wh_comm* c, const char* what )
	{
		if( c->timeout <= 0.0 )
		{
			WH_HIP( hipStreamSynchronize( c->stream ) );
			return 0;
		}
		const auto t0 = std::chrono::steady_clock::now();
		for( long spins = 0;; spins++ )
		{
			const hipError_t e = hipStreamQuery( c->stream );
			if( e == hipSuccess ) return 0;
			if( e != hipErrorNotReady ) return hipFail( e, what, __FILE__, __LINE__ );
			(void)hipGetLastError();
			if( std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count() > c->timeout )
			{
				char buf[ 160 ];
				snprintf( buf, sizeof( buf ), "%s: rank %d of %d gave up after %.0f s (a rank did not arrive)", what, c->rank, c->world, c->timeout );
				setError( buf );
				return WH_E_TIMEOUT;
			}
			if( spins > 64 ) std::this_thread::sleep_for( std::chrono::microseconds( 200 ) );
		}
	}
}

// Packaging check, callable without a GPU: is the collective library there under one of the names wh_comm_* opens, with every entry point they use?
// (The first multi-GPU lease must not fail before its first timed step for a reason a single-GPU box could have shown.)
int wh_comm_runtime_check( char* detail, size_t detailCap )
{
	RcclApi* r = rccl();
	const bool ok = r->lib && r->why.empty() && r->getUniqueId && r->commInitRank && r->commDestroy && r->broadcast && r->allReduce && r->errorString;
	int version = 0;
	if( ok && r->getVersion ) (void)r->getVersion( &version );
	if( detail && detailCap )
	{
		if( ok ) snprintf( detail, detailCap, "opened as %s, version %d, ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclBroadcast / ncclAllReduce / ncclGetErrorString resolved",
			r->loadedAs.c_str(), version );
		else snprintf( detail, detailCap, "%s", r->why.empty() ? "librccl.so: an entry point is missing" : r->why.c_str() );
	}
	if( !ok ) { setError( r->why.empty() ? "librccl.so: an entry point is missing" : r->why ); return WH_E_NOT_READY; }
	return 0;
}

int wh_comm_unique_id( void* id128 )
{
	if( !id128 ) { setError( "comm_unique_id: null argument" ); return WH_E_INVALIDARG; }
	RcclApi* r = rccl();
	if( !r->getUniqueId ) { setError( "comm_unique_id: " + r->why ); return WH_E_NO_DEVICE; }
	const int rc = r->getUniqueId( id128 );
	return rc == 0 ? 0 : rcclFail( rc, "ncclGetUniqueId" );
}

int wh_comm_create( const void* id128, int rank, int worldSize, wh_comm** out )
{
	return wh_comm_create_timeout( id128, rank, worldSize, 0.0, out );
}

int wh_comm_create_timeout( const void* id128, int rank, int worldSize, double timeoutSeconds, wh_comm** out )
{
	if( !id128 || !out || worldSize <= 0 || rank < 0 || rank >= worldSize ) { setError( "comm_create: bad argument" ); return WH_E_INVALIDARG; }
	RcclApi* r = rccl();
	if( !r->commInitRank || !r->broadcast || !r->commDestroy ) { setError( "comm_create: " + r->why ); return WH_E_NO_DEVICE; }
	wh_comm* c = new wh_comm();
	c->rank = rank; c->world = worldSize;
	c->timeout = timeoutSeconds > 0.0 ? timeoutSeconds : 0.0;
	ncclUniqueIdBlob id;
	memcpy( id.internal, id128, WH_COMM_ID_BYTES );
	int rc = 0;
	if( c->timeout <= 0.0 )
		rc = r->commInitRank( &c->comm, worldSize, id, rank );		// uses the calling thread's current device
	else
	{
		// ncclCommInitRank blocks until every rank has called it. With a deadline it runs on a helper thread (bound to the caller's
		// device); when the deadline passes the call returns WH_E_TIMEOUT and the helper is left behind -- the process is expected to
		// exit (whisper-mgpu does), nothing else can be done with a rendezvous that never completes.
		int device = 0;
		WH_HIP( hipGetDevice( &device ) );
		struct Rendezvous { std::mutex mx; std::condition_variable cv; bool done = false; int rc = 0; void* comm = nullptr; };
		auto rv = std::make_shared<Rendezvous>();
		std::thread( [ rv, r, worldSize, id, rank, device ]() {
			(void)hipSetDevice( device );
			void* comm = nullptr;
			const int rcInit = r->commInitRank( &comm, worldSize, id, rank );
			std::lock_guard<std::mutex> lk( rv->mx );
			rv->rc = rcInit; rv->comm = comm; rv->done = true;
			rv->cv.notify_all();
		} ).detach();
		std::unique_lock<std::mutex> lk( rv->mx );
		if( !rv->cv.wait_for( lk, std::chrono::duration<double>( c->timeout ), [ & ]() { return rv->done; } ) )
		{
			char buf[ 160 ];
			snprintf( buf, sizeof( buf ), "ncclCommInitRank: rank %d of %d gave up after %.0f s (a rank did not arrive)", rank, worldSize, c->timeout );
			setError( buf );
			delete c;
			return WH_E_TIMEOUT;
		}
		rc = rv->rc;
		c->comm = rv->comm;
	}
	if( rc != 0 ) { delete c; return rcclFail( rc, "ncclCommInitRank" ); }
	hipError_t e = hipStreamCreateWithFlags( &c->stream, hipStreamNonBlocking );
	if( e == hipSuccess ) e = hipMalloc( (void**)&c->scratch, 8 );
	if( e == hipSuccess ) e = hipMemset( c->scratch, 0, 8 );
	if( e != hipSuccess ) { (void)wh_comm_destroy( c ); return hipFail( e, "comm_create", __FILE__, __LINE__ ); }
	*out = c;
	return 0;
}

int wh_comm_destroy( wh_comm* c )
{
	if( !c ) return 0;
	if( c->stream ) (void)hipStreamSynchronize( c->stream );
	if( c->comm && rccl()->commDestroy ) (void)rccl()->commDestroy( c->comm );
	if( c->scratch ) (void)hipFree( c->scratch );
	if( c->stream ) (void)hipStreamDestroy( c->stream );
	delete c;
	return 0;
}

int wh_comm_info( const wh_comm* c, int* rank, int* worldSize )
{
	if( !c ) { setError( "comm_info: null communicator" ); return WH_E_INVALIDARG; }
	if( rank ) *rank = c->rank;
	if( worldSize ) *worldSize = c->world;
	return 0;
}

int wh_comm_barrier( wh_comm* c )
{
	if( !c ) { setError( "comm_barrier: null communicator" ); return WH_E_INVALIDARG; }
	RcclApi* r = rccl();
	if( !r->allReduce ) { setError( "comm_barrier: " + r->why ); return WH_E_NO_DEVICE; }
	const int rc = r->allReduce( c->scratch, c->scratch + 1, 1, 2 /* ncclInt32 */, 0 /* ncclSum */, c->comm, c->stream );
	if( rc != 0 ) return rcclFail( rc, "ncclAllReduce" );
	return waitComm( c, "comm_barrier" );
}

int wh_comm_set_timeout( wh_comm* c, double seconds )
{
	if( !c ) { setError( "comm_set_timeout: null communicator" ); return WH_E_INVALIDARG; }
	c->timeout = seconds > 0.0 ? seconds : 0.0;
	return 0;
}

int wh_comm_broadcast_i32( wh_comm* c, int root, int32_t* value )
{
	if( !c || !value || root < 0 || root >= c->world ) { setError( "comm_broadcast_i32: bad argument" ); return WH_E_INVALIDARG; }
	RcclApi* r = rccl();
	if( !r->broadcast ) { setError( "comm_broadcast_i32: " + r->why ); return WH_E_NO_DEVICE; }
	if( c->rank == root ) WH_HIP( hipMemcpyAsync( c->scratch, value, 4, hipMemcpyHostToDevice, c->stream ) );
	const int rc = r->broadcast( c->scratch, c->scratch, 4, 0 /* ncclInt8 */, root, c->comm, c->stream );
	if( rc != 0 ) return rcclFail( rc, "ncclBroadcast" );
	WH_CHECK( waitComm( c, "comm_broadcast_i32" ) );
	WH_HIP( hipMemcpy( value, c->scratch, 4, hipMemcpyDeviceToHost ) );
	WH_HIP( hipMemset( c->scratch, 0, 8 ) );
	return 0;
}

int wh_model_broadcast( wh_model* m, wh_comm* c, int root, double* secondsOut )
{
	if( !m || !c || root < 0 || root >= c->world ) { setError( "model_broadcast: bad argument" ); return WH_E_INVALIDARG; }
	if( c->rank == root && !m->finalized ) { setError( "model_broadcast: the root's model is not finalized" ); return WH_E_NOT_READY; }
	WH_BIND( m );
	RcclApi* r = rccl();
	const int64_t bytes = wh_model_arena_bytes( &m->hp );
	WH_HIP( hipDeviceSynchronize() );	   // the root's uploads (synchronous copies on the null stream) are behind us on every stream
	const auto t0 = std::chrono::steady_clock::now();
	const int rc = r->broadcast( m->arena, m->arena, (size_t)bytes, 0 /* ncclInt8 */, root, c->comm, c->stream );
	if( rc != 0 ) return rcclFail( rc, "ncclBroadcast" );
	WH_CHECK( waitComm( c, "model_broadcast" ) );
	if( secondsOut ) *secondsOut = std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count();
	if( c->rank != root )
	{
		// the image holds everything wh_model_finalize builds on the root (derived tables live in the arena)
		m->finalized = true;
		m->filtersSet = true;
	}
	return 0;
}

}	// extern "C"
