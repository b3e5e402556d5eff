// PCM of any rate, sample format and channel count -> mono FP32 at 16 kHz on the GPU.
//
// Replaces the part of the reference's Media Foundation layer that needs nothing from the OS (Whisper/MF/loadAudioFile.cpp, PcmReader.cpp: the source
// reader is configured for 16 kHz float and the OS resamples): rational polyphase resampling with a Kaiser-windowed sinc.
//   g = gcd( Fin, 16000 ), L = 16000 / g, M = Fin / g;  w = ROLLOFF * min( Fin, 16000 ) / Fin  (cutoff as a fraction of the input Nyquist)
//   half = ceil( ZEROS / w ), K = 2 half + 2 taps per phase;  tap k of phase p, d = k - half - p / L, x = d / ( half + 1 ):
//   h[p][k] = w sinc( w d ) I0( BETA sqrt( 1 - x^2 ) ) / I0( BETA ), 0 where |x| >= 1; double on the host, rounded once to float, [L][K]
//   y[n] = sum_k h[p][k] x[base - half + k],  base = ( n M ) div L, p = ( n M ) mod L, x zero outside [0, nFrames);  nOut = ceil( nFrames L / M )
// The sum is FP64: a float * float product is exact in double, one fma per tap in ascending k, one rounding to float at the end, so an output is the
// correctly rounded sum up to ~1e-14 whatever the block shape -- two implementations of the text above agree to the last bit but for such ties.
//
// Kernel: a workgroup owns `block` consecutive outputs of one buffer. The input span they need (block M / L + K frames) is converted from the file's
// own format, downmixed and staged in LDS with zeros outside the buffer; a thread owns up to four outputs (four independent fma chains). The taps of
// all L phases go through LDS as well, K in chunks of kc (a lane reading its own phase's row from global memory touches 64 cache lines per wave
// instruction); tables of more phases than the option resample_lds_phases (rates that share no large factor with 16000) are read from global memory directly.
// LDS is at most 64 KiB per workgroup, so two or more fit a CU at every rate.
// What the kernel shares with the per-chunk kernel of a live stream (capture.hip) -- the design, the block shape, the conversion of a frame and the per-output
// sum -- is stated in resample_device.h; the tap tables live here.
#include "runtime.h"
#include "resample_device.h"

namespace wh
{
	namespace
	{
		struct ResampleArgs
		{
			const void* src;
			float* dst;
			const float* taps;
			long long nFrames, nOut, dstStride;
			int format, channels, channel;
			int L, M, half, K;
			int block;	   // outputs per workgroup, <= RS_BLOCK_MAX
			int xCap;	   // floats of LDS in front of the taps
			int kc, kcp;   // taps per staged chunk and the row pitch of the staged chunk (odd: the phases of neighbouring lanes fall into different banks)
		};

		template<bool TAPS_LDS>
		__global__ void __launch_bounds__( RS_THREADS ) resampleKernel( const ResampleArgs a )
		{
			extern __shared__ __attribute__( ( aligned( 16 ) ) ) float rsLds[];
			float* const xs = rsLds;
			float* const ts = rsLds + a.xCap;

			const int tid = threadIdx.x;
			const long long n0 = (long long)blockIdx.x * a.block;
			const long long left = a.nOut - n0;
			const int count = left < a.block ? (int)left : a.block;
			const long long base0 = ( n0 * a.M ) / a.L;
			const long long first = base0 - a.half;		// input frame of xs[ 0 ]
			int span = (int)( ( ( n0 + count - 1 ) * a.M ) / a.L - base0 ) + a.K;
			span = span < a.xCap ? span : a.xCap;		// the launcher sized `block` so that this never cuts
			for( int i = tid; i < span; i += RS_THREADS )
			{
				const long long g = first + i;
				xs[ i ] = ( g >= 0 && g < a.nFrames ) ? loadFrame( a.src, g, a.format, a.channels, a.channel ) : 0.0f;
			}

			// outputs tid, tid + 256, ... of the block; an idle slot (j >= count) walks the block's first K inputs with phase 0 and stores nothing
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
				if( j < count ) a.dst[ ( n0 + j ) * a.dstStride ] = (float)acc[ o ];
			}
		}

		// 16 kHz in: conversion and downmix only
		__global__ void __launch_bounds__( RS_THREADS ) pcmConvertKernel( const void* __restrict__ src, int format, int channels, int channel, long long nFrames,
			float* __restrict__ dst, long long dstStride )
		{
			for( long long i = (long long)blockIdx.x * RS_THREADS + threadIdx.x; i < nFrames; i += (long long)gridDim.x * RS_THREADS )
				dst[ i * dstStride ] = loadFrame( src, i, format, channels, channel );
		}

		// ---- the filter, on the host ----
		using Design = ResampleDesign;
		bool design( int inRate, Design& d ) { return resampleDesign( inRate, d ); }
		// modified Bessel function of the first kind, order 0: the power series (all terms positive, x <= 15: ~40 terms to double precision)
		double besselI0( double x )
		{
			const double q = 0.25 * x * x;
			double term = 1.0, sum = 1.0;
			for( int k = 1; k < 500; k++ )
			{
				term *= q / ( (double)k * (double)k );
				sum += term;
				if( term < sum * 1e-18 ) break;
			}
			return sum;
		}
		void designTaps( int inRate, const Design& d, float* taps )
		{
			const double PI = 3.14159265358979323846;
			const double w = RS_ROLLOFF * (double)( inRate < RS_OUT_RATE ? inRate : RS_OUT_RATE ) / (double)inRate;
			const double i0Beta = besselI0( RS_BETA );
			for( int p = 0; p < d.L; p++ )
				for( int k = 0; k < d.K; k++ )
				{
					const double dist = (double)( k - d.half ) - (double)p / (double)d.L;
					const double x = dist / ( (double)d.half + 1.0 );
					double h = 0.0;
					if( std::fabs( x ) < 1.0 )
					{
						const double t = PI * w * dist;
						const double sinc = t == 0.0 ? 1.0 : std::sin( t ) / t;
						h = w * sinc * ( besselI0( RS_BETA * std::sqrt( 1.0 - x * x ) ) / i0Beta );
					}
					taps[ (size_t)p * d.K + k ] = (float)h;
				}
		}

		int64_t outLen( const Design& d, int64_t nFrames ) { return resampleOutLen( d, nFrames ); }

		bool validCall( const char* who, int format, int channels, int channel, int inRate, int64_t nFrames, int64_t dstStride, int64_t nOut, Design& d )
		{
			if( !design( inRate, d ) ) { setError( std::string( who ) + ": the rate must be 1000 .. 384000 Hz" ); return false; }
			if( format < WH_PCM_U8 || format > WH_PCM_F32 ) { setError( std::string( who ) + ": unknown sample format" ); return false; }
			if( channels < 1 || channels > RS_MAX_CHANNELS || channel < -1 || channel >= channels ) { setError( std::string( who ) + ": 1 .. 8 channels, channel -1 .. channels - 1" ); return false; }
			if( dstStride != 1 && dstStride != 2 ) { setError( std::string( who ) + ": dstStride must be 1 or 2" ); return false; }
			if( nFrames < 0 || nFrames > ( (int64_t)1 << 40 ) || nOut != outLen( d, nFrames ) ) { setError( std::string( who ) + ": nOut must be wh_resample_out_len( inRate, nFrames )" ); return false; }
			return true;
		}
	}	// namespace

	// The tap tables: one per (device, rate), built on first use under the lock and kept for the life of the process like the op-level scratch of
	// ops_debug.hip. A table is L * K floats: 119 KB at 44.1 kHz, 175 KB at 11.025 kHz, 104 MB at worst (a rate coprime to 16000: L = 16000).
	namespace
	{
		std::mutex g_tapMutex;
		std::map<std::pair<int, int>, ResampleTapTable> g_tapTables;
		std::vector<Allocation> g_tapAllocations;
	}

	int resampleTapTable( int inRate, hipStream_t stream, ResampleTapTable& out )
	{
		int dev = 0;
		WH_HIP( hipGetDevice( &dev ) );
		std::lock_guard<std::mutex> lk( g_tapMutex );
		const auto it = g_tapTables.find( { dev, inRate } );
		if( it != g_tapTables.end() ) { out = it->second; return 0; }
		ResampleTapTable t;
		if( !design( inRate, t.d ) ) return WH_E_INVALIDARG;
		std::vector<float> host( (size_t)t.d.L * t.d.K );
		designTaps( inRate, t.d, host.data() );
		Allocation a;
		WH_HIP( guardedAlloc( a, (int64_t)host.size() * 4, -1, "resample taps", stream ) );
		// synchronous: `host` dies with this call, and every stream may read the table afterwards
		hipError_t e = hipMemcpyAsync( a.body, host.data(), host.size() * 4, hipMemcpyHostToDevice, stream );
		if( e == hipSuccess ) e = hipStreamSynchronize( stream );
		if( e != hipSuccess ) { (void)guardedFree( a ); return hipFail( e, "resample taps upload", __FILE__, __LINE__ ); }
		g_tapAllocations.push_back( a );
		t.dev = (const float*)a.body;
		g_tapTables[ { dev, inRate } ] = t;
		out = t;
		return 0;
	}

	int launchResample( hipStream_t stream, const void* src, int format, int channels, int channel, int inRate, long long nFrames, float* dst,
		long long dstStride, long long nOut )
	{
		if( nOut <= 0 ) return 0;
		if( inRate == RS_OUT_RATE )
		{
			const long long blocks = ( nFrames + RS_THREADS - 1 ) / RS_THREADS;
			hipLaunchKernelGGL( pcmConvertKernel, dim3( (unsigned)( blocks < 65536 ? blocks : 65536 ) ), dim3( RS_THREADS ), 0, stream, src, format, channels, channel,
				nFrames, dst, dstStride );
			WH_HIP( hipGetLastError() );
			return 0;
		}
		ResampleTapTable t;
		WH_CHECK( resampleTapTable( inRate, stream, t ) );
		const Design& d = t.d;
		ResampleShape sh;
		if( !resampleShape( d, sh ) ) { setError( "resample: internal error (block span)" ); return WH_E_BOUNDS; }
		ResampleArgs a;
		a.src = src; a.dst = dst; a.taps = t.dev;
		a.nFrames = nFrames; a.nOut = nOut; a.dstStride = dstStride;
		a.format = format; a.channels = channels; a.channel = channel;
		a.L = d.L; a.M = d.M; a.half = d.half; a.K = d.K;
		a.block = sh.block; a.xCap = sh.xCap; a.kc = sh.kc; a.kcp = sh.kcp;
		const long long block = sh.block;
		const bool tapsLds = sh.tapsLds;
		const size_t lds = sh.ldsBytes;
		const long long blocks = ( nOut + block - 1 ) / block;
		if( blocks > 0x7fffffffll ) { setError( "resample: too many outputs for one launch" ); return WH_E_INVALIDARG; }
		if( tapsLds ) hipLaunchKernelGGL( resampleKernel<true>, dim3( (unsigned)blocks ), dim3( RS_THREADS ), lds, stream, a );
		else hipLaunchKernelGGL( resampleKernel<false>, dim3( (unsigned)blocks ), dim3( RS_THREADS ), lds, stream, a );
		WH_HIP( hipGetLastError() );
		return 0;
	}
}	// namespace wh

extern "C" {

int wh_resample_out_len( int inRate, int64_t nFrames, int64_t* nOut )
{
	Design d;
	if( !nOut || nFrames < 0 || nFrames > ( (int64_t)1 << 40 ) || !design( inRate, d ) )
	{
		setError( "resample_out_len: the rate must be 1000 .. 384000 Hz, nFrames 0 .. 2^40" );
		return WH_E_INVALIDARG;
	}
	*nOut = outLen( d, nFrames );
	return 0;
}

int wh_resample_taps( int inRate, int32_t* L, int32_t* M, int32_t* half, int32_t* K, float* tapsHost, int64_t cap )
{
	Design d;
	if( !design( inRate, d ) ) { setError( "resample_taps: the rate must be 1000 .. 384000 Hz" ); return WH_E_INVALIDARG; }
	if( L ) *L = d.L;
	if( M ) *M = d.M;
	if( half ) *half = d.half;
	if( K ) *K = d.K;
	if( !tapsHost ) return 0;
	if( cap < (int64_t)d.L * d.K ) { setError( "resample_taps: the buffer holds fewer than L * K floats" ); return WH_E_INVALIDARG; }
	designTaps( inRate, d, tapsHost );
	return 0;
}

int wh_resample( void* stream, const void* srcDev, int format, int channels, int channel, int inRate, int64_t nFrames, float* dstDev, int64_t dstStride,
	int64_t nOut )
{
	Design d;
	if( !validCall( "resample", format, channels, channel, inRate, nFrames, dstStride, nOut, d ) ) return WH_E_INVALIDARG;
	if( nFrames == 0 ) return 0;
	const uintptr_t align = format == WH_PCM_S16 ? 1 : ( format == WH_PCM_S32 || format == WH_PCM_F32 ) ? 3 : 0;
	if( !srcDev || !dstDev || ( (uintptr_t)srcDev & align ) != 0 || ( (uintptr_t)dstDev & 3 ) != 0 )
	{
		setError( "resample: null or misaligned buffer" );
		return WH_E_INVALIDARG;
	}
	return launchResample( (hipStream_t)stream, srcDev, format, channels, channel, inRate, nFrames, dstDev, dstStride, nOut );
}

int wh_resample_host_multi( const void* src, int format, int channels, const int32_t* channelList, int count, int inRate, int64_t nFrames, float* const* dsts,
	const int64_t* dstStrides, int64_t nOut )
{
	if( !channelList || !dsts || !dstStrides || count < 1 || count > 16 ) { setError( "resample_host: 1 .. 16 results" ); return WH_E_INVALIDARG; }
	Design d;
	for( int i = 0; i < count; i++ )
		if( !validCall( "resample_host", format, channels, channelList[ i ], inRate, nFrames, dstStrides[ i ], nOut, d ) ) return WH_E_INVALIDARG;
	if( nFrames == 0 ) return 0;
	for( int i = 0; i < count; i++ )
		if( !dsts[ i ] ) { setError( "resample_host: null buffer" ); return WH_E_INVALIDARG; }
	if( !src ) { setError( "resample_host: null buffer" ); return WH_E_INVALIDARG; }
	const int64_t srcBytes = nFrames * channels * ( format == WH_PCM_U8 ? 1 : format == WH_PCM_S16 ? 2 : format == WH_PCM_S24 ? 3 : 4 );
	// one upload of the file's own samples, one result buffer of `count` rows, one download
	Allocation in = { nullptr, nullptr, 0, nullptr }, out = in;
	hipError_t e = guardedAlloc( in, srcBytes, -1, "resample source", nullptr );
	if( e == hipSuccess ) e = guardedAlloc( out, nOut * 4 * count, -1, "resample result", nullptr );
	int rc = 0;
	std::vector<float> packed;
	if( e == hipSuccess ) e = hipMemcpyAsync( in.body, src, (size_t)srcBytes, hipMemcpyHostToDevice, nullptr );
	for( int i = 0; i < count && e == hipSuccess && rc == 0; i++ )
		rc = launchResample( nullptr, in.body, format, channels, channelList[ i ], inRate, nFrames, (float*)out.body + (int64_t)i * nOut, 1, nOut );
	if( e == hipSuccess && rc == 0 )
	{
		const bool direct = count == 1 && dstStrides[ 0 ] == 1;
		float* host = dsts[ 0 ];
		if( !direct ) { packed.resize( (size_t)nOut * count ); host = packed.data(); }
		e = hipMemcpyAsync( host, out.body, (size_t)nOut * 4 * count, hipMemcpyDeviceToHost, nullptr );
		if( e == hipSuccess ) e = hipStreamSynchronize( nullptr );
		if( e == hipSuccess && !direct )
			for( int i = 0; i < count; i++ )
				for( int64_t n = 0; n < nOut; n++ ) dsts[ i ][ n * dstStrides[ i ] ] = packed[ (size_t)( i * nOut + n ) ];
	}
	else if( e == hipSuccess ) (void)hipStreamSynchronize( nullptr );
	if( e != hipSuccess ) rc = hipFail( e, "resample_host", __FILE__, __LINE__ );
	int bad = 0;
	if( in.base ) bad += guardedFree( in ) > 0;
	if( out.base ) bad += guardedFree( out ) > 0;
	if( rc == 0 && bad ) { setError( "resample_host: a guard region of a device buffer was written" ); rc = WH_E_BOUNDS; }
	return rc;
}

int wh_resample_host( const void* src, int format, int channels, int channel, int inRate, int64_t nFrames, float* dst, int64_t dstStride, int64_t nOut )
{
	const int32_t list[ 1 ] = { channel };
	float* const dsts[ 1 ] = { dst };
	const int64_t strides[ 1 ] = { dstStride };
	return wh_resample_host_multi( src, format, channels, list, 1, inRate, nFrames, dsts, strides, nOut );
}

}	// extern "C"
