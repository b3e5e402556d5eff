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
//
// A stream at another rate R (wh_capture_create_rate) is resampled by the same launch, with wh_resample's filter made resumable. With L, M, half, K and the
// taps of R (resample.hip), output n of the whole stream is y[n] = sum_k h[p][k] x[base - half + k], base = ( n M ) div L, p = ( n M ) mod L, FP64, one fma
// per tap in ascending k, rounded once: resampleChains of resample_device.h, which resampleKernel calls too. A stream holds nIn (input frames accepted),
// nOut (outputs emitted or skipped), z (frames below it read as zero) and the last K - 1 input frames of every filtered channel as floats:
//   append( F )  nIn += F; outputs [nOut, max( nOut, ready )) go to the buffer at n, ready = max( 0, ceil( ( nIn - half - 1 ) L / M ) ) = the outputs whose last
//                tap lies inside what has arrived. The first output that is not ready has base >= nIn - half - 1 and reaches back to nIn - ( K - 1 ) at most.
//   flush()      outputs [nOut, ceil( nIn L / M )) with x = 0 from nIn on: half + 1 frames of zeros behind the history. The total is wh_resample_out_len( R, nIn ).
//   skip( F )    nIn += F; nOut = max( nOut, ceil( nIn L / M ) ); z = nIn. Host arithmetic only: the kernel reads every frame below z as zero, the history too.
// nOut == max( ready( nIn ), ceil( z L / M ) ) at all times, which is how the op-level entry gets it from nIn and z.
// Kernel: captureRateKernel keeps captureAppendKernel's form and ownership. A workgroup computes the outputs of this append that fall into its tile of 4096 buffer
// positions, in blocks of resampleKernel's shape (at most 1024 outputs): the input span of a block is staged in LDS from the history (stream frames
// [nIn - ( K - 1 ), nIn)) and the chunk behind it, once per filtered channel -- the downmix, and channels 0 and 1 when the stereo of a two-channel source is kept.
// The outputs go to the device buffer, the pinned mirror and, times 32768, straight into the VadTile. The history is two buffers: every workgroup reads one,
// workgroup 0 writes the other (the last K - 1 frames of old history + chunk, which for a chunk shorter than K - 1 is the old one's tail and the chunk).
// LDS: the VadTile (36 KiB) and resampleKernel's staging (up to 62 KiB) side by side, one workgroup per CU; an append launches one to five workgroups.
#include "runtime.h"
#include "vad_device.h"
#include "resample_device.h"
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

		// ---- a stream at another rate ----
		struct CaptureRateArgs
		{
			const void* src;			   // the chunk, device, interleaved; not read by a flush
			float *mono, *stereo;
			float *monoHost, *stereoHost;
			const double* twiddles;
			const float* taps;
			const float* histRead;		   // [nf][K - 1]: stream frames [nIn - ( K - 1 ), nIn) of every filtered channel
			float* histWrite;			   // the same for nIn + frames; not written by a flush
			float* feat;
			long long n, count;			   // buffer position before the append, outputs of the append
			long long o0;				   // the first of them as an output of the stream
			long long nIn, frames, z;	   // input frames in front of the chunk, frames of the chunk (flush: 0), resume point
			long long tile0;
			int format, channels, nf, flush;
			int L, M, half, K;
			int block, xCap, kc, kcp;
		};

		// stream frame g of filtered channel c (0: the downmix, or the only channel; 1, 2: channels 0, 1)
		__device__ __forceinline__ float captureRateInput( const CaptureRateArgs& a, int c, long long g )
		{
			const long long h0 = a.nIn - ( a.K - 1 );
			if( g < a.z || g < h0 ) return 0.0f;
			if( g < a.nIn ) return a.histRead[ (long long)c * ( a.K - 1 ) + ( g - h0 ) ];
			if( a.flush || g >= a.nIn + a.frames ) return 0.0f;
			return loadFrame( a.src, g - a.nIn, a.format, a.channels, c == 0 ? ( a.channels == 2 ? -1 : 0 ) : c - 1 );
		}

		template<bool TAPS_LDS>
		__global__ void __launch_bounds__( VAD_THREADS ) captureRateKernel( const CaptureRateArgs a )
		{
			static_assert( VAD_THREADS == RS_THREADS && sizeof( VadTile ) % 16 == 0, "one workgroup shape for both halves" );
			extern __shared__ __attribute__( ( aligned( 16 ) ) ) unsigned char capLds[];
			VadTile& t = *(VadTile*)capLds;
			float* const xs = (float*)( capLds + sizeof( VadTile ) );
			float* const ts = xs + a.xCap;

			const int tid = threadIdx.x;
			const long long tile = a.tile0 + blockIdx.x, s0 = tile * CAP_TILE, end = a.n + a.count;
			const long long newLo = a.n / VAD_N, newHi = end / VAD_N;
			const long long loL = newLo - tile * VAD_FR, hiL = newHi - tile * VAD_FR;
			const int lo = loL < 0 ? 0 : ( loL > VAD_FR ? VAD_FR : (int)loL ), hi = hiL < 0 ? 0 : ( hiL > VAD_FR ? VAD_FR : (int)hiL );
			for( int i = tid; i < 2 * VAD_N; i += VAD_THREADS ) ( &t.tw[ 0 ][ 0 ] )[ i ] = a.twiddles[ i ];
			// the older part of a frame that began in an earlier append; the new part is written below, everything else is zeros
			for( int i = tid; i < CAP_TILE; i += VAD_THREADS )
			{
				const int f = i >> 8;
				const long long s = s0 + i;
				const bool old = f >= lo && f < hi && s < a.n;
				t.xs[ f * VAD_X_STRIDE + ( i & 255 ) ] = old ? __fmul_rn( a.mono[ s ], 32768.0f ) : 0.0f;
			}

			// the history of the next append: the last K - 1 frames of what this one has seen
			if( blockIdx.x == 0 && !a.flush )
				for( int i = tid; i < a.nf * ( a.K - 1 ); i += VAD_THREADS )
				{
					const int c = i / ( a.K - 1 ), j = i - c * ( a.K - 1 );
					a.histWrite[ i ] = captureRateInput( a, c, a.nIn + a.frames - ( a.K - 1 ) + j );
				}

			// the outputs of this append inside the tile, as buffer positions
			const long long pLo = s0 > a.n ? s0 : a.n, pHi = s0 + CAP_TILE < end ? s0 + CAP_TILE : end;
			for( int c = 0; c < a.nf; c++ )
				for( long long b0 = pLo; b0 < pHi; b0 += a.block )
				{
					const int count = pHi - b0 < a.block ? (int)( pHi - b0 ) : a.block;
					const long long n0 = a.o0 + ( b0 - a.n );
					const long long base0 = ( n0 * a.M ) / a.L;
					const long long first = base0 - a.half;		// stream frame of xs[ 0 ]
					int span = (int)( ( ( n0 + count - 1 ) * a.M ) / a.L - base0 ) + a.K;
					span = span < a.xCap ? span : a.xCap;		// resampleShape sized `block` so that this never cuts
					__syncthreads();							// the block before has read xs
					for( int i = tid; i < span; i += VAD_THREADS ) xs[ i ] = captureRateInput( a, c, first + i );
					int off[ RS_PER_THREAD ], ph[ RS_PER_THREAD ];
					double acc[ RS_PER_THREAD ];
#pragma unroll
					for( int o = 0; o < RS_PER_THREAD; o++ )
					{
						const int j = tid + o * RS_THREADS;
						off[ o ] = ph[ o ] = 0;
						acc[ o ] = 0.0;
						if( j < count )
						{
							const long long nm = ( n0 + j ) * a.M, base = nm / a.L;
							ph[ o ] = (int)( nm - base * a.L );
							off[ o ] = (int)( base - base0 );
						}
					}
					__syncthreads();
					resampleChains<TAPS_LDS>( xs, ts, a.taps, a.L, a.K, a.kc, a.kcp, off, ph, acc );
#pragma unroll
					for( int o = 0; o < RS_PER_THREAD; o++ )
					{
						const int j = tid + o * RS_THREADS;
						if( j >= count ) continue;
						const long long s = b0 + j;
						const float v = (float)acc[ o ];
						if( c == 0 )
						{
							a.mono[ s ] = v;
							if( a.monoHost ) a.monoHost[ s ] = v;
							const int i = (int)( s - s0 ), f = i >> 8;
							if( f >= lo && f < hi ) t.xs[ f * VAD_X_STRIDE + ( i & 255 ) ] = __fmul_rn( v, 32768.0f );
						}
						if( a.stereo && ( c > 0 || a.nf == 1 ) )
						{
							// a mono source whose stereo is kept gets its one filtered channel twice
							const long long e0 = 2 * s + ( c > 0 ? c - 1 : 0 ), e1 = c > 0 ? e0 : e0 + 1;
							a.stereo[ e0 ] = v;
							a.stereo[ e1 ] = v;
							if( a.stereoHost ) { a.stereoHost[ e0 ] = v; a.stereoHost[ e1 ] = v; }
						}
					}
				}
			if( lo >= hi ) return;	  // uniform over the workgroup: nothing to compute
			__syncthreads();
			vadTileFeatures( t, lo, hi, a.feat, tile * VAD_FR - newLo );
		}

		constexpr int64_t CAP_MAX_FRAMES = (int64_t)1 << 40;
		constexpr int CAP_RATE_LDS_MAX = (int)sizeof( VadTile ) + ( RS_X_CAP + RS_T_CAP ) * 4;

		// ready: the outputs whose last tap lies inside nIn frames
		int64_t readyOutputs( const ResampleDesign& d, int64_t nIn )
		{
			const int64_t t = nIn - d.half - 1;
			return t <= 0 ? 0 : ( t * d.L + d.M - 1 ) / d.M;
		}
		// the outputs an append of `frames` frames (flush: the end of the stream) adds to a stream at nIn, nOut
		int64_t rateOutputs( const ResampleDesign& d, int64_t nIn, int64_t nOut, int64_t frames, bool flush )
		{
			const int64_t target = flush ? resampleOutLen( d, nIn ) : readyOutputs( d, nIn + frames );
			return target > nOut ? target - nOut : 0;
		}

		// every argument checked by the caller; a.n, a.count, a.o0, a.nIn, a.frames, a.z, the buffers, format, channels, nf and flush are set
		int launchCaptureRate( hipStream_t stream, int inRate, CaptureRateArgs& a )
		{
			ResampleTapTable t;
			WH_CHECK( resampleTapTable( inRate, stream, t ) );
			ResampleShape sh;
			if( !resampleShape( t.d, sh ) ) { setError( "capture: internal error (block span)" ); return WH_E_BOUNDS; }
			WH_CHECK( vadTable( stream, a.twiddles ) );
			a.taps = t.dev;
			a.L = t.d.L; a.M = t.d.M; a.half = t.d.half; a.K = t.d.K;
			a.block = sh.block; a.xCap = sh.xCap; a.kc = sh.kc; a.kcp = sh.kcp;
			a.tile0 = a.n / CAP_TILE;
			// a chunk that makes no output ready still moves the history: one workgroup
			const long long tiles = a.count > 0 ? ( a.n + a.count - 1 ) / CAP_TILE - a.tile0 + 1 : 1;
			const size_t lds = sizeof( VadTile ) + sh.ldsBytes;
			if( sh.tapsLds ) return launchLds<captureRateKernel<true>, CAP_RATE_LDS_MAX>( dim3( (unsigned)tiles ), dim3( VAD_THREADS ), lds, stream, a );
			return launchLds<captureRateKernel<false>, CAP_RATE_LDS_MAX>( dim3( (unsigned)tiles ), dim3( VAD_THREADS ), lds, stream, a );
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
	// a stream at another rate than 16 kHz (wh_capture_create_rate); nothing of it is allocated at 16 kHz
	int inRate = 16000, nf = 1;
	ResampleDesign d = { 1, 1, 0, 0 };
	int64_t nIn = 0, nOut = 0, z = 0;
	bool flushed = false;
	Allocation hist[ 2 ] = { { nullptr, nullptr, 0, nullptr }, { nullptr, nullptr, 0, nullptr } };
	int histCur = 0;	 // the one the next launch reads
};

namespace
{
	// wh_capture_append and wh_capture_flush of a stream at another rate: one upload (not for a flush), one launch, one download of the features
	int appendRate( const char* who, wh_capture* p, const void* src, int format, int64_t frames, bool flush, float* featHost, int64_t featCap, int64_t* nNewFrames )
	{
		if( p->flushed ) { setError( std::string( who ) + ": the stream was flushed" ); return WH_E_NOT_READY; }
		if( frames > CAP_MAX_FRAMES - p->nIn ) { setError( std::string( who ) + ": more than 2^40 frames in one stream" ); return WH_E_INVALIDARG; }
		const int64_t count = rateOutputs( p->d, p->nIn, p->nOut, frames, flush );
		if( count > p->cap - p->n ) { setError( std::string( who ) + ": the chunk does not fit the buffer" ); return WH_E_BOUNDS; }
		const int64_t nNew = ( p->n + count ) / VAD_N - p->n / VAD_N;
		if( featCap < nNew || ( nNew > 0 && !featHost ) ) { setError( std::string( who ) + ": featHost holds fewer than the completed frames" ); return WH_E_INVALIDARG; }
		*nNewFrames = 0;
		if( flush && count == 0 ) { p->flushed = true; return 0; }
		if( !flush && frames == 0 ) return 0;
		WH_HIP( hipSetDevice( p->device ) );
		if( !flush )
		{
			const size_t bytes = (size_t)frames * p->channels * ( format == WH_PCM_S16 ? 2 : 4 );
			if( (int64_t)bytes > p->chunk.bytes )
			{
				// every append waited for its launch: nothing uses the old staging
				if( guardedFree( p->chunk ) > 0 ) { p->chunk = { nullptr, nullptr, 0, nullptr }; setError( std::string( who ) + ": a guard region of the staging buffer was written" ); return WH_E_BOUNDS; }
				p->chunk = { nullptr, nullptr, 0, nullptr };
				WH_HIP( guardedAlloc( p->chunk, (int64_t)bytes, -1, "capture chunk", p->stream ) );
			}
			WH_HIP( hipMemcpyAsync( p->chunk.body, src, bytes, hipMemcpyHostToDevice, p->stream ) );
		}
		CaptureRateArgs a;
		a.src = p->chunk.body;
		a.mono = (float*)p->mono.body;
		a.stereo = (float*)p->stereo.body;
		a.monoHost = p->monoHostDev[ p->cur ];
		a.stereoHost = p->keepStereo ? p->stereoHostDev[ p->cur ] : nullptr;
		a.histRead = (const float*)p->hist[ p->histCur ].body;
		a.histWrite = (float*)p->hist[ p->histCur ^ 1 ].body;
		a.feat = (float*)p->feat.body;
		a.n = p->n;
		a.count = count;
		a.o0 = p->nOut;
		a.nIn = p->nIn;
		a.frames = flush ? 0 : frames;
		a.z = p->z;
		a.format = format;
		a.channels = p->channels;
		a.nf = p->nf;
		a.flush = flush ? 1 : 0;
		WH_CHECK( launchCaptureRate( p->stream, p->inRate, a ) );
		if( nNew > 0 ) WH_HIP( hipMemcpyAsync( featHost, p->feat.body, (size_t)nNew * 3 * 4, hipMemcpyDeviceToHost, p->stream ) );
		// its own stream only: a transcription on a context's stream goes on
		WH_HIP( hipStreamSynchronize( p->stream ) );
		if( flush ) p->flushed = true;
		else
		{
			p->nIn += frames;
			p->histCur ^= 1;
		}
		p->nOut += count;
		p->n += count;
		*nNewFrames = nNew;
		return 0;
	}

	int createCapture( const char* who, wh_context* c, int channels, int keepStereo, int64_t capSamples, int inRate, wh_capture** out )
	{
		if( !c || !out || ( channels != 1 && channels != 2 ) || capSamples < VAD_N || capSamples > CAP_MAX_SAMPLES )
		{
			setError( std::string( who ) + ": 1 or 2 channels, capSamples 256 .. 2^30" );
			return WH_E_INVALIDARG;
		}
		ResampleDesign d = { 1, 1, 0, 0 };
		if( inRate != 16000 && !resampleDesign( inRate, d ) ) { setError( std::string( who ) + ": the rate must be 1000 .. 384000 Hz" ); return WH_E_INVALIDARG; }
		*out = nullptr;
		WH_BIND( c->m );
		wh_capture* p = new wh_capture();
		p->device = c->m->device;
		p->channels = channels;
		p->keepStereo = keepStereo != 0;
		p->cap = capSamples;
		p->inRate = inRate;
		p->d = d;
		p->nf = channels == 2 && p->keepStereo ? 3 : 1;
		int rc = 0;
		hipError_t e = hipStreamCreateWithFlags( &p->stream, hipStreamNonBlocking );
		if( e == hipSuccess ) e = guardedAlloc( p->mono, capSamples * 4, 0, "capture mono", p->stream );
		if( e == hipSuccess && p->keepStereo ) e = guardedAlloc( p->stereo, capSamples * 8, 0, "capture stereo", p->stream );
		// the staging of a chunk in its own format: a second of f32 to begin with, grown by the first larger chunk
		if( e == hipSuccess ) e = guardedAlloc( p->chunk, std::min<int64_t>( capSamples, 16000 ) * channels * 4, -1, "capture chunk", p->stream );
		if( e == hipSuccess ) e = guardedAlloc( p->feat, ( capSamples / VAD_N + 1 ) * 3 * 4, -1, "capture features", p->stream );
		for( int i = 0; i < 2 && e == hipSuccess && inRate != 16000; i++ ) e = guardedAlloc( p->hist[ i ], (int64_t)p->nf * ( d.K - 1 ) * 4, 0, "capture history", p->stream );
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
		if( e != hipSuccess ) rc = hipFail( e, who, __FILE__, __LINE__ );
		if( rc != 0 ) { (void)wh_capture_destroy( p ); return rc; }
		*out = p;
		return 0;
	}
}

extern "C" {

int wh_capture_create( wh_context* c, int channels, int keepStereo, int64_t capSamples, wh_capture** out )
{
	return createCapture( "capture_create", c, channels, keepStereo, capSamples, 16000, out );
}

int wh_capture_create_rate( wh_context* c, int channels, int keepStereo, int64_t capSamples, int inRate, wh_capture** out )
{
	return createCapture( "capture_create_rate", c, channels, keepStereo, capSamples, inRate, out );
}

int wh_capture_destroy( wh_capture* p )
{
	if( !p ) return 0;
	(void)hipSetDevice( p->device );
	if( p->stream ) (void)hipStreamSynchronize( p->stream );
	int bad = 0;
	for( const Allocation* a : { &p->mono, &p->stereo, &p->chunk, &p->feat, &p->hist[ 0 ], &p->hist[ 1 ] } )
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
	if( p->inRate != 16000 ) return appendRate( "capture_append", p, src, format, frames, false, featHost, featCap, nNewFrames );
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

int wh_capture_flush( wh_capture* p, float* featHost, int64_t featCap, int64_t* nNewFrames )
{
	if( !p || !nNewFrames ) { setError( "capture_flush: null pointer" ); return WH_E_INVALIDARG; }
	// at 16 kHz every sample is in the buffer already
	if( p->inRate == 16000 ) { *nNewFrames = 0; return 0; }
	return appendRate( "capture_flush", p, nullptr, WH_PCM_S16, 0, true, featHost, featCap, nNewFrames );
}

int wh_capture_skip( wh_capture* p, int64_t frames, int64_t* nSkippedOutputs )
{
	if( !p || !nSkippedOutputs || frames < 0 || frames > CAP_MAX_FRAMES - p->nIn ) { setError( "capture_skip: frames 0 .. 2^40, non-null pointers" ); return WH_E_INVALIDARG; }
	if( p->inRate == 16000 ) { *nSkippedOutputs = frames; return 0; }
	if( p->flushed ) { setError( "capture_skip: the stream was flushed" ); return WH_E_NOT_READY; }
	p->nIn += frames;
	const int64_t upTo = resampleOutLen( p->d, p->nIn );
	*nSkippedOutputs = upTo > p->nOut ? upTo - p->nOut : 0;
	p->nOut += *nSkippedOutputs;
	// the kernel reads every frame below z as zero, the history too
	p->z = p->nIn;
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

int wh_op_capture_append_rate( void* stream, const void* srcDev, int format, int channels, int inRate, int64_t frames, int64_t nIn, int64_t z, int flush,
	const float* histReadDev, float* histWriteDev, int64_t n, int64_t capSamples, float* monoDev, float* stereoDev, float* featDev, int64_t* nOutputs )
{
	ResampleDesign d;
	if( inRate == 16000 || !resampleDesign( inRate, d ) )
	{
		setError( "op_capture_append_rate: the rate must be 1000 .. 384000 Hz and not 16000 (wh_op_capture_append)" );
		return WH_E_INVALIDARG;
	}
	if( !validFormat( format, channels ) || !nOutputs || n < 0 || frames < 0 || nIn < 0 || nIn > CAP_MAX_FRAMES || frames > CAP_MAX_FRAMES - nIn || z < 0 || z > nIn ||
		capSamples < 0 || capSamples > CAP_MAX_SAMPLES || ( flush && frames != 0 ) )
	{
		setError( "op_capture_append_rate: format s16 or f32, 1 or 2 channels, n, frames >= 0, 0 <= z <= nIn <= 2^40, capSamples 0 .. 2^30, no frames with a flush" );
		return WH_E_INVALIDARG;
	}
	*nOutputs = 0;
	// the stream's invariant: every ready output was emitted, and a skip moved past the outputs in front of z
	const int64_t ready = readyOutputs( d, nIn ), skipped = resampleOutLen( d, z ), nOut = ready > skipped ? ready : skipped;
	const int64_t count = rateOutputs( d, nIn, nOut, frames, flush != 0 );
	if( n > capSamples || count > capSamples - n ) { setError( "op_capture_append_rate: the outputs do not fit the buffer" ); return WH_E_BOUNDS; }
	if( flush ? count == 0 : frames == 0 ) return 0;
	const int64_t nNew = ( n + count ) / VAD_N - n / VAD_N;
	const uintptr_t align = format == WH_PCM_S16 ? 1 : 3;
	if( ( !flush && !srcDev ) || !monoDev || !histReadDev || ( !flush && !histWriteDev ) || histReadDev == histWriteDev || ( nNew > 0 && !featDev ) ||
		( (uintptr_t)srcDev & align ) != 0 || ( (uintptr_t)monoDev & 3 ) != 0 || ( (uintptr_t)stereoDev & 3 ) != 0 || ( (uintptr_t)featDev & 3 ) != 0 ||
		( (uintptr_t)histReadDev & 3 ) != 0 || ( (uintptr_t)histWriteDev & 3 ) != 0 )
	{
		setError( "op_capture_append_rate: null or misaligned buffer, or one history buffer for both" );
		return WH_E_INVALIDARG;
	}
	CaptureRateArgs a;
	a.src = srcDev;
	a.mono = monoDev;
	a.stereo = stereoDev;
	a.monoHost = a.stereoHost = nullptr;
	a.histRead = histReadDev;
	a.histWrite = histWriteDev;
	a.feat = featDev;
	a.n = n;
	a.count = count;
	a.o0 = nOut;
	a.nIn = nIn;
	a.frames = frames;
	a.z = z;
	a.format = format;
	a.channels = channels;
	a.nf = channels == 2 && stereoDev ? 3 : 1;
	a.flush = flush ? 1 : 0;
	WH_CHECK( launchCaptureRate( (hipStream_t)stream, inRate, a ) );
	*nOutputs = count;
	return 0;
}

}	// extern "C"
