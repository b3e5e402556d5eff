// A live PCM stream on the GPU, chunk by chunk: what the capture loop of iContext::runCapture (Whisper/Whisper/ContextImpl.capture.cpp:290-358 readSample,
// :391-395 detectVoice) does per read -- append the converted samples to the buffer, then look for voice in it -- as ONE launch per chunk.
//
// The buffer is 16 kHz mono FP32 on the device (and interleaved stereo when kept), position n. A chunk of `frames` sample frames in the caller's own
// format (s16 or f32, 1 or 2 channels) becomes samples [n, n + frames) by wh_resample's rules for inRate == 16000: s16 is v / 32768, f32 as is, mono of
// two channels the FP32 sum in channel order times 0.5f, a mono source whose stereo is kept gets its channel twice. The chunk completes the 256-sample
// frames [n / 256, ( n + frames ) / 256) of the buffer; their voice-activity features are wh_vad_features's bits for the same 256 samples.
//
// Kernel: ownership follows vadFeaturesKernel's tile. A workgroup owns 16 consecutive frames of BUFFER positions (4096 samples): it converts whatever part
// of the chunk falls into them -- to the device buffer and, through mapped pinned memory, to the host mirror --, stages the frames the chunk completes in
// LDS (samples in front of n come from the buffer: earlier launches on the same stream wrote them, no workgroup of this launch does) and calls
// vadTileFeatures of vad_device.h. A workgroup reads nothing another workgroup of the same launch writes, so no grid-wide ordering is needed.
#include "runtime.h"
#include "vad_device.h"
#include <algorithm>

namespace wh
{
	namespace
	{
		constexpr int CAP_TILE = VAD_FR * VAD_N;	   // samples a workgroup owns
		constexpr int64_t CAP_MAX_SAMPLES = (int64_t)1 << 30;

		struct CaptureArgs
		{
			const void* src;			   // the chunk, device, interleaved
			float *mono, *stereo;		   // the device buffer; stereo may be null
			float *monoHost, *stereoHost;  // device addresses of the pinned mirror; null at op level
			const double* twiddles;
			float* feat;				   // [newHi - newLo][3]
			long long n, frames;		   // buffer position before the chunk, sample frames of the chunk
			long long tile0;			   // first tile the chunk touches
			int format, channels;
		};

		__device__ __forceinline__ float captureSample( const void* src, long long i, int format )
		{
			return format == WH_PCM_S16 ? (float)( (const int16_t*)src )[ i ] / 32768.0f : ( (const float*)src )[ i ];
		}

		__global__ void __launch_bounds__( VAD_THREADS ) captureAppendKernel( const CaptureArgs a )
		{
			__shared__ VadTile t;

			const int tid = threadIdx.x;
			const long long tile = a.tile0 + blockIdx.x, s0 = tile * CAP_TILE, end = a.n + a.frames;
			// the frames this chunk completes, as frames of the tile
			const long long newLo = a.n / VAD_N, newHi = end / VAD_N;
			const long long loL = newLo - tile * VAD_FR, hiL = newHi - tile * VAD_FR;
			const int lo = loL < 0 ? 0 : ( loL > VAD_FR ? VAD_FR : (int)loL ), hi = hiL < 0 ? 0 : ( hiL > VAD_FR ? VAD_FR : (int)hiL );
			for( int i = tid; i < 2 * VAD_N; i += VAD_THREADS ) ( &t.tw[ 0 ][ 0 ] )[ i ] = a.twiddles[ i ];
			for( int i = tid; i < CAP_TILE; i += VAD_THREADS )
			{
				const int f = i >> 8;
				const long long s = s0 + i;
				const bool wanted = f >= lo && f < hi;
				float v = 0.0f;
				if( s >= a.n && s < end )
				{
					const long long k = s - a.n;
					float l, r;
					if( a.channels == 2 )
					{
						l = captureSample( a.src, 2 * k, a.format );
						r = captureSample( a.src, 2 * k + 1, a.format );
						v = __fmul_rn( __fadd_rn( l, r ), 0.5f );
					}
					else v = l = r = captureSample( a.src, k, a.format );
					a.mono[ s ] = v;
					if( a.monoHost ) a.monoHost[ s ] = v;
					if( a.stereo )
					{
						a.stereo[ 2 * s ] = l;
						a.stereo[ 2 * s + 1 ] = r;
						if( a.stereoHost )
						{
							a.stereoHost[ 2 * s ] = l;
							a.stereoHost[ 2 * s + 1 ] = r;
						}
					}
				}
				else if( wanted && s < a.n ) v = a.mono[ s ];	  // the older part of a frame that began in an earlier chunk
				// a frame that this chunk does not complete is all zeros: its features are dropped
				t.xs[ f * VAD_X_STRIDE + ( i & 255 ) ] = wanted ? __fmul_rn( v, 32768.0f ) : 0.0f;
			}
			if( lo >= hi ) return;	  // uniform over the workgroup: nothing to compute
			__syncthreads();
			vadTileFeatures( t, lo, hi, a.feat, tile * VAD_FR - newLo );
		}

		bool validFormat( int format, int channels ) { return ( format == WH_PCM_S16 || format == WH_PCM_F32 ) && ( channels == 1 || channels == 2 ); }

		// every argument checked by the caller: n >= 0, frames > 0, n + frames inside the buffers
		int launchCaptureAppend( hipStream_t stream, CaptureArgs& a )
		{
			WH_CHECK( vadTable( stream, a.twiddles ) );
			a.tile0 = a.n / CAP_TILE;
			const long long tiles = ( a.n + a.frames - 1 ) / CAP_TILE - a.tile0 + 1;
			hipLaunchKernelGGL( captureAppendKernel, dim3( (unsigned)tiles ), dim3( VAD_THREADS ), 0, stream, a );
			WH_HIP( hipGetLastError() );
			return 0;
		}
	}	// namespace
}	// namespace wh

struct wh_capture
{
	int device = 0, channels = 1;
	bool keepStereo = false;
	int64_t cap = 0, n = 0;
	hipStream_t stream = nullptr;
	Allocation mono = { nullptr, nullptr, 0, nullptr }, stereo = mono, chunk = mono, feat = mono;
	// the pinned mirror, twice: wh_capture_take hands one out and the next piece fills the other
	float *monoHost[ 2 ] = { nullptr, nullptr }, *stereoHost[ 2 ] = { nullptr, nullptr };
	float *monoHostDev[ 2 ] = { nullptr, nullptr }, *stereoHostDev[ 2 ] = { nullptr, nullptr };
	int cur = 0;
};

extern "C" {

int wh_capture_create( wh_context* c, int channels, int keepStereo, int64_t capSamples, wh_capture** out )
{
	if( !c || !out || ( channels != 1 && channels != 2 ) || capSamples < VAD_N || capSamples > CAP_MAX_SAMPLES )
	{
		setError( "capture_create: 1 or 2 channels, capSamples 256 .. 2^30" );
		return WH_E_INVALIDARG;
	}
	*out = nullptr;
	WH_BIND( c->m );
	wh_capture* p = new wh_capture();
	p->device = c->m->device;
	p->channels = channels;
	p->keepStereo = keepStereo != 0;
	p->cap = capSamples;
	int rc = 0;
	hipError_t e = hipStreamCreateWithFlags( &p->stream, hipStreamNonBlocking );
	if( e == hipSuccess ) e = guardedAlloc( p->mono, capSamples * 4, 0, "capture mono", p->stream );
	if( e == hipSuccess && p->keepStereo ) e = guardedAlloc( p->stereo, capSamples * 8, 0, "capture stereo", p->stream );
	// the staging of a chunk in its own format: a second of f32 to begin with, grown by the first larger chunk
	if( e == hipSuccess ) e = guardedAlloc( p->chunk, std::min<int64_t>( capSamples, 16000 ) * channels * 4, -1, "capture chunk", p->stream );
	if( e == hipSuccess ) e = guardedAlloc( p->feat, ( capSamples / VAD_N + 1 ) * 3 * 4, -1, "capture features", p->stream );
	for( int i = 0; i < 2 && e == hipSuccess; i++ )
	{
		e = hipHostMalloc( (void**)&p->monoHost[ i ], (size_t)capSamples * 4, hipHostMallocMapped | hipHostMallocCoherent );
		if( e == hipSuccess ) e = hipHostGetDevicePointer( (void**)&p->monoHostDev[ i ], p->monoHost[ i ], 0 );
		if( e == hipSuccess && p->keepStereo )
		{
			e = hipHostMalloc( (void**)&p->stereoHost[ i ], (size_t)capSamples * 8, hipHostMallocMapped | hipHostMallocCoherent );
			if( e == hipSuccess ) e = hipHostGetDevicePointer( (void**)&p->stereoHostDev[ i ], p->stereoHost[ i ], 0 );
		}
	}
	if( e == hipSuccess ) e = hipStreamSynchronize( p->stream );
	if( e != hipSuccess ) rc = hipFail( e, "capture_create", __FILE__, __LINE__ );
	if( rc != 0 ) { (void)wh_capture_destroy( p ); return rc; }
	*out = p;
	return 0;
}

int wh_capture_destroy( wh_capture* p )
{
	if( !p ) return 0;
	(void)hipSetDevice( p->device );
	if( p->stream ) (void)hipStreamSynchronize( p->stream );
	int bad = 0;
	for( const Allocation* a : { &p->mono, &p->stereo, &p->chunk, &p->feat } )
		if( a->base ) bad += guardedFree( *a ) > 0;
	for( int i = 0; i < 2; i++ )
	{
		if( p->monoHost[ i ] ) (void)hipHostFree( p->monoHost[ i ] );
		if( p->stereoHost[ i ] ) (void)hipHostFree( p->stereoHost[ i ] );
	}
	if( p->stream ) (void)hipStreamDestroy( p->stream );
	delete p;
	if( bad ) { setError( "capture_destroy: a guard region of a device buffer was written" ); return WH_E_BOUNDS; }
	return 0;
}

int wh_capture_append( wh_capture* p, const void* src, int format, int64_t frames, float* featHost, int64_t featCap, int64_t* nNewFrames )
{
	if( !p || !nNewFrames || frames < 0 || !validFormat( format, p->channels ) || ( frames > 0 && !src ) )
	{
		setError( "capture_append: format s16 or f32, frames >= 0, non-null buffers" );
		return WH_E_INVALIDARG;
	}
	if( frames > p->cap - p->n ) { setError( "capture_append: the chunk does not fit the buffer" ); return WH_E_BOUNDS; }
	const int64_t nNew = ( p->n + frames ) / VAD_N - p->n / VAD_N;
	if( featCap < nNew || ( nNew > 0 && !featHost ) ) { setError( "capture_append: featHost holds fewer than the completed frames" ); return WH_E_INVALIDARG; }
	*nNewFrames = 0;
	if( frames == 0 ) return 0;
	WH_HIP( hipSetDevice( p->device ) );
	const size_t bytes = (size_t)frames * p->channels * ( format == WH_PCM_S16 ? 2 : 4 );
	if( (int64_t)bytes > p->chunk.bytes )
	{
		// every append waited for its launch: nothing uses the old staging
		if( guardedFree( p->chunk ) > 0 ) { p->chunk = { nullptr, nullptr, 0, nullptr }; setError( "capture_append: a guard region of the staging buffer was written" ); return WH_E_BOUNDS; }
		p->chunk = { nullptr, nullptr, 0, nullptr };
		WH_HIP( guardedAlloc( p->chunk, (int64_t)bytes, -1, "capture chunk", p->stream ) );
	}
	WH_HIP( hipMemcpyAsync( p->chunk.body, src, bytes, hipMemcpyHostToDevice, p->stream ) );
	CaptureArgs a;
	a.src = p->chunk.body;
	a.mono = (float*)p->mono.body;
	a.stereo = (float*)p->stereo.body;
	a.monoHost = p->monoHostDev[ p->cur ];
	a.stereoHost = p->keepStereo ? p->stereoHostDev[ p->cur ] : nullptr;
	a.feat = (float*)p->feat.body;
	a.n = p->n;
	a.frames = frames;
	a.format = format;
	a.channels = p->channels;
	WH_CHECK( launchCaptureAppend( p->stream, a ) );
	if( nNew > 0 ) WH_HIP( hipMemcpyAsync( featHost, p->feat.body, (size_t)nNew * 3 * 4, hipMemcpyDeviceToHost, p->stream ) );
	// its own stream only: a transcription on a context's stream goes on
	WH_HIP( hipStreamSynchronize( p->stream ) );
	p->n += frames;
	*nNewFrames = nNew;
	return 0;
}

int wh_capture_clear( wh_capture* p )
{
	if( !p ) { setError( "capture_clear: null capture" ); return WH_E_INVALIDARG; }
	p->n = 0;
	return 0;
}

int wh_capture_take( wh_capture* p, const float** monoHost, const float** stereoHost, int64_t* nSamples )
{
	if( !p || !monoHost || !nSamples ) { setError( "capture_take: null pointer" ); return WH_E_INVALIDARG; }
	// every append waited for its launch: the mirror is complete
	*monoHost = p->monoHost[ p->cur ];
	if( stereoHost ) *stereoHost = p->keepStereo ? p->stereoHost[ p->cur ] : nullptr;
	*nSamples = p->n;
	p->cur ^= 1;
	p->n = 0;
	return 0;
}

int wh_capture_size( const wh_capture* p, int64_t* nSamples )
{
	if( !p || !nSamples ) { setError( "capture_size: null pointer" ); return WH_E_INVALIDARG; }
	*nSamples = p->n;
	return 0;
}

int wh_op_capture_append( void* stream, const void* srcDev, int format, int channels, int64_t n, int64_t frames, int64_t capSamples, float* monoDev,
	float* stereoDev, float* featDev )
{
	if( !validFormat( format, channels ) || n < 0 || frames < 0 || capSamples < 0 || capSamples > CAP_MAX_SAMPLES )
	{
		setError( "op_capture_append: format s16 or f32, 1 or 2 channels, n, frames >= 0, capSamples 0 .. 2^30" );
		return WH_E_INVALIDARG;
	}
	if( n > capSamples || frames > capSamples - n ) { setError( "op_capture_append: the chunk does not fit the buffer" ); return WH_E_BOUNDS; }
	if( frames == 0 ) return 0;
	const int64_t nNew = ( n + frames ) / VAD_N - n / VAD_N;
	const uintptr_t align = format == WH_PCM_S16 ? 1 : 3;
	if( !srcDev || !monoDev || ( nNew > 0 && !featDev ) || ( (uintptr_t)srcDev & align ) != 0 || ( (uintptr_t)monoDev & 3 ) != 0 || ( (uintptr_t)stereoDev & 3 ) != 0 ||
		( (uintptr_t)featDev & 3 ) != 0 )
	{
		setError( "op_capture_append: null or misaligned buffer" );
		return WH_E_INVALIDARG;
	}
	CaptureArgs a;
	a.src = srcDev;
	a.mono = monoDev;
	a.stereo = stereoDev;
	a.monoHost = a.stereoHost = nullptr;
	a.feat = featDev;
	a.n = n;
	a.frames = frames;
	a.format = format;
	a.channels = channels;
	return launchCaptureAppend( (hipStream_t)stream, a );
}

}	// extern "C"
