// What the two resampling kernels share, stated once: resampleKernel (resample.hip, a whole buffer) and captureRateKernel (capture.hip, the outputs a chunk
// of a live stream makes ready) stage an input span in LDS each in its own way and then run resampleChains, so an output is the same bits whichever kernel
// formed it. Here: the design of a rate (L, M, half, K), the tap table per (device, rate), the shape of a block of outputs, the conversion of one frame
// and the per-output fma chain. resample.hip's header has the text of the filter and owns the tables.
#pragma once
#include "runtime.h"

namespace wh
{
	constexpr int RS_THREADS = 256, RS_PER_THREAD = 4, RS_BLOCK_MAX = RS_THREADS * RS_PER_THREAD;
	constexpr int RS_X_CAP = 8192;	  // floats of staged input per workgroup
	constexpr int RS_T_CAP = 7680;	  // floats of staged taps per workgroup: 62 KiB with the input, under the 64 KiB a launch gets without asking
	constexpr int RS_MIN_RATE = 1000, RS_MAX_RATE = 384000, RS_OUT_RATE = 16000, RS_MAX_CHANNELS = 8;
	constexpr int RS_ZEROS = 32;
	constexpr double RS_ROLLOFF = 0.9475937167399596, RS_BETA = 14.769656459379492;

	// ---- the design of a rate, on the host ----
	struct ResampleDesign { int L, M, half, K; };
	inline int resampleGcd( int a, int b ) { while( b ) { const int t = a % b; a = b; b = t; } return a; }
	inline bool resampleDesign( int inRate, ResampleDesign& d )
	{
		if( inRate < RS_MIN_RATE || inRate > RS_MAX_RATE ) return false;
		const int g = resampleGcd( inRate, RS_OUT_RATE );
		d.L = RS_OUT_RATE / g;
		d.M = inRate / g;
		const double w = RS_ROLLOFF * (double)( inRate < RS_OUT_RATE ? inRate : RS_OUT_RATE ) / (double)inRate;
		d.half = (int)std::ceil( (double)RS_ZEROS / w );
		d.K = 2 * d.half + 2;
		return true;
	}
	inline int64_t resampleOutLen( const ResampleDesign& d, int64_t nFrames ) { return ( nFrames * d.L + d.M - 1 ) / d.M; }

	// The tap table of a rate on the calling thread's current device (resample.hip): [L][K] floats, built and uploaded by the first call, kept for the life of the process
	struct ResampleTapTable { ResampleDesign d; const float* dev; };
	int resampleTapTable( int inRate, hipStream_t stream, ResampleTapTable& out );

	// The shape of a workgroup's block of outputs and of its LDS, from the design alone
	struct ResampleShape
	{
		int block;	   // outputs per block, <= RS_BLOCK_MAX
		int xCap;	   // floats of LDS in front of the taps
		int kc, kcp;   // taps per staged chunk and the row pitch of the staged chunk (odd: the phases of neighbouring lanes fall into different banks); 0: taps from global memory
		bool tapsLds;
		size_t ldsBytes;
	};
	inline bool resampleShape( const ResampleDesign& d, ResampleShape& s )
	{
		// the span of `block` outputs is at most ceil( ( block - 1 ) M / L ) + K frames: the largest multiple of 64 that fits RS_X_CAP (K <= 1624, M / L <= 24: 64 always fit)
		long long block = ( (long long)( RS_X_CAP - d.K - 1 ) * d.L / d.M + 1 ) / 64 * 64;
		block = block > RS_BLOCK_MAX ? RS_BLOCK_MAX : ( block < 64 ? 64 : block );
		s.block = (int)block;
		s.xCap = (int)( ( ( block - 1 ) * d.M + d.L - 1 ) / d.L ) + d.K;
		if( s.xCap > RS_X_CAP ) return false;
		s.xCap = ( s.xCap + 3 ) & ~3;
		// taps through LDS when a chunk of at least 8 taps of every phase fits
		const int maxRow = ( ( RS_T_CAP / d.L ) - 1 ) | 1;
		s.tapsLds = RS_T_CAP / d.L >= 9 && d.L <= g_opt.resampleLdsPhases;
		s.kc = s.kcp = 0;
		if( s.tapsLds )
		{
			s.kc = d.K < maxRow ? d.K : maxRow;
			s.kcp = s.kc | 1;
		}
		s.ldsBytes = ( (size_t)s.xCap + ( s.tapsLds ? (size_t)d.L * s.kcp : 0 ) ) * sizeof( float );
		return true;
	}

	// ---- one frame as a float ----
	__device__ __forceinline__ float loadSample( const uint8_t* p, int format )
	{
		switch( format )
		{
		case WH_PCM_U8: return (float)( (int)*p - 128 ) / 128.0f;
		case WH_PCM_S16: return (float)*(const int16_t*)p / 32768.0f;
		case WH_PCM_S24:
		{
			const int v = (int)( ( (unsigned)p[ 0 ] | ( (unsigned)p[ 1 ] << 8 ) | ( (unsigned)p[ 2 ] << 16 ) ) << 8 ) >> 8;
			return (float)v / 8388608.0f;
		}
		case WH_PCM_S32: return (float)( (double)*(const int32_t*)p * ( 1.0 / 2147483648.0 ) );
		default: return *(const float*)p;
		}
	}
	__device__ __forceinline__ int sampleBytes( int format ) { return format == WH_PCM_U8 ? 1 : format == WH_PCM_S16 ? 2 : format == WH_PCM_S24 ? 3 : 4; }

	// one frame as a mono float: channel >= 0 that channel, -1 the mean -- the FP32 sum in channel order times 1.0f / C (two channels: the bits of 0.5f * ( l + r ))
	__device__ __forceinline__ float loadFrame( const void* src, long long frame, int format, int channels, int channel )
	{
		const int bytes = sampleBytes( format );
		const uint8_t* p = (const uint8_t*)src + ( frame * channels + ( channel < 0 ? 0 : channel ) ) * bytes;
		if( channel >= 0 ) return loadSample( p, format );
		float s = loadSample( p, format );
		for( int c = 1; c < channels; c++ ) s = __fadd_rn( s, loadSample( p + c * bytes, format ) );
		return __fmul_rn( s, 1.0f / (float)channels );
	}

	// ---- the per-output sum ----
	// Called by all RS_THREADS threads of the workgroup behind the barrier that follows the staging of xs. A thread owns up to four outputs: output o reads the
	// staged input from xs[ off[ o ] ] on with the taps of phase ph[ o ], FP64, one fma per tap in ascending k; an idle slot has off = ph = 0 and its sum is
	// dropped by the caller. TAPS_LDS: the taps of all L phases go through ts, K in chunks of kc, row pitch kcp; otherwise they are read from `taps` directly.
	// Ends behind a barrier when TAPS_LDS, so that the caller may stage again.
	template<bool TAPS_LDS>
	__device__ __forceinline__ void resampleChains( const float* xs, float* ts, const float* __restrict__ taps, int L, int K, int kc, int kcp,
		const int ( &off )[ RS_PER_THREAD ], const int ( &ph )[ RS_PER_THREAD ], double ( &acc )[ RS_PER_THREAD ] )
	{
		const int tid = threadIdx.x;
		if( TAPS_LDS )
		{
			for( int k0 = 0; k0 < K; k0 += kc )
			{
				const int kn = K - k0 < kc ? K - k0 : kc;
				for( int r = tid / 32; r < L; r += RS_THREADS / 32 )
					for( int kk = tid & 31; kk < kn; kk += 32 ) ts[ r * kcp + kk ] = taps[ (long long)r * K + k0 + kk ];
				__syncthreads();
				const float *t0 = ts + ph[ 0 ] * kcp, *t1 = ts + ph[ 1 ] * kcp, *t2 = ts + ph[ 2 ] * kcp, *t3 = ts + ph[ 3 ] * kcp;
				const float *x0 = xs + off[ 0 ] + k0, *x1 = xs + off[ 1 ] + k0, *x2 = xs + off[ 2 ] + k0, *x3 = xs + off[ 3 ] + k0;
				for( int kk = 0; kk < kn; kk++ )
				{
					acc[ 0 ] = fma( (double)t0[ kk ], (double)x0[ kk ], acc[ 0 ] );
					acc[ 1 ] = fma( (double)t1[ kk ], (double)x1[ kk ], acc[ 1 ] );
					acc[ 2 ] = fma( (double)t2[ kk ], (double)x2[ kk ], acc[ 2 ] );
					acc[ 3 ] = fma( (double)t3[ kk ], (double)x3[ kk ], acc[ 3 ] );
				}
				__syncthreads();
			}
		}
		else
		{
			const float *t0 = taps + (long long)ph[ 0 ] * K, *t1 = taps + (long long)ph[ 1 ] * K, *t2 = taps + (long long)ph[ 2 ] * K, *t3 = taps + (long long)ph[ 3 ] * K;
			const float *x0 = xs + off[ 0 ], *x1 = xs + off[ 1 ], *x2 = xs + off[ 2 ], *x3 = xs + off[ 3 ];
			for( int k = 0; k < K; k++ )
			{
				acc[ 0 ] = fma( (double)t0[ k ], (double)x0[ k ], acc[ 0 ] );
				acc[ 1 ] = fma( (double)t1[ k ], (double)x1[ k ], acc[ 1 ] );
				acc[ 2 ] = fma( (double)t2[ k ], (double)x2[ k ], acc[ 2 ] );
				acc[ 3 ] = fma( (double)t3[ k ], (double)x3[ k ], acc[ 3 ] );
			}
		}
	}
}	// namespace wh
