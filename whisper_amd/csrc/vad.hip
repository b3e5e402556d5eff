// Voice-activity features of 16 kHz mono PCM on the GPU: what a chunk planner needs to cut a long recording at pauses.
//
// Replaces the per-frame half of VAD::detect (Whisper/Whisper/voiceActivityDetection.cpp:65-113, :145-155; Moattar & Homayounpour 2009). Frame f is
// samples [256 f, 256 f + 256), the last partial frame is ignored; with x[n] = pcm[n] * 32768.0f and X the 256-point DFT of x:
//   energy = sqrtf( (float)( sum_n (double)(float)( x[n] x[n] ) / 256 ) )
//   F      = 62.5f * the first k in 0 .. 127 that maximises |X[k]|^2
//   SFM    = -10 log10( (float)( exp( sum_{k<256} ln|X[k]| / 256 ) / ( sum_{k<256} |X[k]| / 256 ) ) )
// The reference evaluates X with a recursive FP32 FFT over approximate sines; here X is the direct DFT in FP64 against a host-built twiddle table, i.e. the
// exact value the reference approximates, every sum is FP64 in a fixed order and each feature is rounded to float once (the square root and the final
// logarithm are the correctly rounded float functions: evaluated in double on a float argument). A frame's three numbers depend on its 256 samples only --
// not on its place in a workgroup, nor on the length of the buffer.
//
// Kernel: the DFT is a GEMM [frames][256] x [256][bins] on v_mfma_f64_16x16x4_f64, as in melKernelMf. A workgroup of four waves takes VAD_FR = 16 frames
// (one M tile); a real input has |X[256 - k]| = |X[k]|, so only bins 0 .. 128 are formed and the two 256-bin sums are |X0| + |X128| + 2 sum_{1 .. 127}.
// Bins 0 and 128 are real (their sine column is zero), so bin 128 rides in the unused imaginary accumulator of bin 0: that column's second operand is
// cos( pi n ) instead of -sin( 0 ), and 8 tiles of 16 bins cover all 129. A wave owns tiles `wave` and `wave + 4`: four accumulator chains per A operand.
// |X|^2 goes to LDS [16][129]; then a wave reduces four frames, a lane two bins of each (lane 0 a third), through xor butterflies -- no atomics, and lane 0
// writes the frame's three floats.
// Everything behind the staging of the 16 frames is vadTileFeatures of vad_device.h, which the capture kernel (capture.hip) calls on its own staging: a frame's
// three floats are the same bits from either kernel.
#include "runtime.h"
#include "vad_device.h"

namespace wh
{
	namespace
	{
		constexpr int64_t VAD_MAX_SAMPLES = (int64_t)1 << 40;

		__global__ void __launch_bounds__( VAD_THREADS ) vadFeaturesKernel( const float* __restrict__ pcm, long long nFrames, const double* __restrict__ twiddles,
			float* __restrict__ feat )
		{
			__shared__ VadTile t;

			const int tid = threadIdx.x;
			const long long f0 = (long long)blockIdx.x * VAD_FR;
			for( int i = tid; i < 2 * VAD_N; i += VAD_THREADS ) ( &t.tw[ 0 ][ 0 ] )[ i ] = twiddles[ i ];
			for( int i = tid; i < VAD_FR * VAD_N; i += VAD_THREADS )
			{
				const int f = i >> 8, n = i & 255;
				// a frame at or beyond nFrames is all zeros: nothing of the ignored tail, nor anything behind the buffer, is read
				t.xs[ f * VAD_X_STRIDE + n ] = f0 + f < nFrames ? __fmul_rn( pcm[ ( f0 + f ) * VAD_N + n ], 32768.0f ) : 0.0f;
			}
			__syncthreads();
			// the arithmetic is vad_device.h's, shared with the capture kernel
			const long long left = nFrames - f0;
			vadTileFeatures( t, 0, left < VAD_FR ? (int)left : VAD_FR, feat, f0 );
		}

		// The twiddle table: one per device, built in double on the host, uploaded on first use under the lock and kept for the life of the process
		// like the resampler's tap tables. 4 KB.
		std::mutex g_vadMutex;
		std::map<int, const double*> g_vadTables;
		std::vector<Allocation> g_vadAllocations;
	}	// namespace

	int vadTable( hipStream_t stream, const double*& out )
	{
		int dev = 0;
		WH_HIP( hipGetDevice( &dev ) );
		std::lock_guard<std::mutex> lk( g_vadMutex );
		const auto it = g_vadTables.find( dev );
		if( it != g_vadTables.end() ) { out = it->second; return 0; }
		const double PI = 3.14159265358979323846;
		std::vector<double> host( 2 * VAD_N );
		for( int i = 0; i < VAD_N; i++ )
		{
			const double t = 2.0 * PI * (double)i / (double)VAD_N;
			host[ i ] = std::cos( t );
			host[ VAD_N + i ] = -std::sin( t );
		}
		// the quarter points exactly: bins 0 and 128 are sums of +-x[n]
		host[ 0 ] = 1.0; host[ 64 ] = 0.0; host[ 128 ] = -1.0; host[ 192 ] = 0.0;
		host[ VAD_N + 0 ] = 0.0; host[ VAD_N + 64 ] = -1.0; host[ VAD_N + 128 ] = 0.0; host[ VAD_N + 192 ] = 1.0;
		Allocation a;
		WH_HIP( guardedAlloc( a, (int64_t)host.size() * 8, -1, "vad twiddles", stream ) );
		// synchronous: `host` dies with this call, and every stream may read the table afterwards
		hipError_t e = hipMemcpyAsync( a.body, host.data(), host.size() * 8, hipMemcpyHostToDevice, stream );
		if( e == hipSuccess ) e = hipStreamSynchronize( stream );
		if( e != hipSuccess ) { (void)guardedFree( a ); return hipFail( e, "vad twiddles upload", __FILE__, __LINE__ ); }
		g_vadAllocations.push_back( a );
		out = g_vadTables[ dev ] = (const double*)a.body;
		return 0;
	}

	namespace
	{
		int launchVadFeatures( hipStream_t stream, const float* pcm, long long nFrames, float* feat )
		{
			if( nFrames <= 0 ) return 0;
			const double* table = nullptr;
			WH_CHECK( vadTable( stream, table ) );
			const long long blocks = ( nFrames + VAD_FR - 1 ) / VAD_FR;
			hipLaunchKernelGGL( vadFeaturesKernel, dim3( (unsigned)blocks ), dim3( VAD_THREADS ), 0, stream, pcm, nFrames, table, feat );
			WH_HIP( hipGetLastError() );
			return 0;
		}
	}	// namespace
}	// namespace wh

extern "C" {

int wh_vad_frame_count( int64_t nSamples, int64_t* nFrames )
{
	if( !nFrames || nSamples < 0 || nSamples > VAD_MAX_SAMPLES ) { setError( "vad_frame_count: nSamples 0 .. 2^40" ); return WH_E_INVALIDARG; }
	*nFrames = nSamples / VAD_N;
	return 0;
}

int wh_vad_features( void* stream, const float* pcmDev, int64_t nSamples, float* featDev )
{
	int64_t nFrames = 0;
	if( 0 != wh_vad_frame_count( nSamples, &nFrames ) ) { setError( "vad_features: nSamples 0 .. 2^40" ); return WH_E_INVALIDARG; }
	if( nFrames == 0 ) return 0;
	if( !pcmDev || !featDev || ( (uintptr_t)pcmDev & 3 ) != 0 || ( (uintptr_t)featDev & 3 ) != 0 ) { setError( "vad_features: null or misaligned buffer" ); return WH_E_INVALIDARG; }
	return launchVadFeatures( (hipStream_t)stream, pcmDev, nFrames, featDev );
}

int wh_vad_features_host( const float* pcm, int64_t nSamples, float* feat )
{
	int64_t nFrames = 0;
	if( 0 != wh_vad_frame_count( nSamples, &nFrames ) ) { setError( "vad_features_host: nSamples 0 .. 2^40" ); return WH_E_INVALIDARG; }
	if( nFrames == 0 ) return 0;
	if( !pcm || !feat ) { setError( "vad_features_host: null buffer" ); return WH_E_INVALIDARG; }
	// the whole frames only: the ignored tail is not uploaded
	Allocation in = { nullptr, nullptr, 0, nullptr }, out = in;
	hipError_t e = guardedAlloc( in, nFrames * VAD_N * 4, -1, "vad source", nullptr );
	if( e == hipSuccess ) e = guardedAlloc( out, nFrames * 3 * 4, -1, "vad features", nullptr );
	int rc = 0;
	if( e == hipSuccess ) e = hipMemcpyAsync( in.body, pcm, (size_t)( nFrames * VAD_N * 4 ), hipMemcpyHostToDevice, nullptr );
	if( e == hipSuccess ) rc = launchVadFeatures( nullptr, (const float*)in.body, nFrames, (float*)out.body );
	if( e == hipSuccess && rc == 0 ) e = hipMemcpyAsync( feat, out.body, (size_t)( nFrames * 3 * 4 ), hipMemcpyDeviceToHost, nullptr );
	if( e == hipSuccess ) e = hipStreamSynchronize( nullptr );
	if( e != hipSuccess ) rc = hipFail( e, "vad_features_host", __FILE__, __LINE__ );
	int bad = 0;
	if( in.base ) bad += guardedFree( in ) > 0;
	if( out.base ) bad += guardedFree( out ) > 0;
	if( rc == 0 && bad ) { setError( "vad_features_host: a guard region of a device buffer was written" ); rc = WH_E_BOUNDS; }
	return rc;
}

}	// extern "C"
