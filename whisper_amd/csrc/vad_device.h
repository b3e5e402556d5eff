// The feature arithmetic of the voice-activity kernels, stated once: vadFeaturesKernel (vad.hip, a whole buffer) and captureAppendKernel (capture.hip, the
// frames a chunk of a live stream completes) stage 16 frames in LDS each in its own way and then call vadTileFeatures, so a frame's three floats are the
// same bits whichever kernel formed them. vad.hip's header explains the tile; this file holds no host code.
#pragma once
#include "common.h"

namespace wh
{
	constexpr int VAD_N = 256, VAD_FR = 16, VAD_THREADS = 256, VAD_WAVES = VAD_THREADS / 64;
	// Frames start 256 floats apart = a multiple of the 32 LDS banks, and the A operand reads one sample of each of the 16 frames per instruction:
	// sample s of the workgroup lives at s + 2 ( s / 256 ), so lane ( frame, kq ) of a half wave reads bank 2 frame + kq + n0 -- 32 different ones.
	constexpr int VAD_X_STRIDE = VAD_N + 2;
	constexpr int VAD_P_STRIDE = 129;	 // |X|^2 of bins 0 .. 128
	typedef double vadF64x4 __attribute__( ( ext_vector_type( 4 ) ) );

	// The LDS of a tile: the twiddles, the 16 frames x[n] = pcm[n] * 32768.0f (a frame that is not wanted: zeros), |X|^2
	struct VadTile
	{
		double tw[ 2 ][ VAD_N ];	  // cos, -sin of 2 pi i / 256
		float xs[ VAD_FR * VAD_X_STRIDE ];
		double pw[ VAD_FR ][ VAD_P_STRIDE ];
	};

	// The twiddle table of the calling thread's current device (vad.hip): built and uploaded by the first call, kept for the life of the process
	int vadTable( hipStream_t stream, const double*& out );

	// Called by all 256 threads of the workgroup behind the barrier that follows the staging of t.tw and t.xs. Frames lo <= f < hi of the tile get their
	// features at feat[ 3 ( outFrame0 + f ) ]; the other frames are computed and dropped.
	__device__ __forceinline__ void vadTileFeatures( VadTile& t, int lo, int hi, float* __restrict__ feat, long long outFrame0 )
	{
		const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
		// ---- DFT bins 0 .. 128: A lane & 15 = frame, lane >> 4 = sample within the 4-deep K step; B lane & 15 = bin, lane >> 4 = sample ----
		const int row = lane & 15, kq = lane >> 4;
		{
			const int bin0 = wave * 16 + row, bin1 = ( wave + VAD_WAVES ) * 16 + row;
			// the column of bin 0 carries bin 128 in its imaginary accumulator: cos( 2 pi ( 128 n ) / 256 ) = cos( pi n )
			const double* const imTab0 = &t.tw[ 0 ][ 0 ] + ( bin0 == 0 ? 0 : VAD_N );
			const int imBin0 = bin0 == 0 ? 128 : bin0;
			int re0i = ( kq * bin0 ) & 255, im0i = ( kq * imBin0 ) & 255, b1i = ( kq * bin1 ) & 255;
			const int re0s = ( 4 * bin0 ) & 255, im0s = ( 4 * imBin0 ) & 255, b1s = ( 4 * bin1 ) & 255;
			const float* const px = t.xs + row * VAD_X_STRIDE + kq;
			vadF64x4 re0 = { 0.0, 0.0, 0.0, 0.0 }, im0 = re0, re1 = re0, im1 = re0;
			for( int n0 = 0; n0 < VAD_N; n0 += 4 )
			{
				const double a = (double)px[ n0 ];
				re0 = __builtin_amdgcn_mfma_f64_16x16x4f64( a, t.tw[ 0 ][ re0i ], re0, 0, 0, 0 );
				im0 = __builtin_amdgcn_mfma_f64_16x16x4f64( a, imTab0[ im0i ], im0, 0, 0, 0 );
				re1 = __builtin_amdgcn_mfma_f64_16x16x4f64( a, t.tw[ 0 ][ b1i ], re1, 0, 0, 0 );
				im1 = __builtin_amdgcn_mfma_f64_16x16x4f64( a, t.tw[ 1 ][ b1i ], im1, 0, 0, 0 );
				re0i = ( re0i + re0s ) & 255;
				im0i = ( im0i + im0s ) & 255;
				b1i = ( b1i + b1s ) & 255;
			}
			// D: column = lane & 15 = bin of the tile, row = ( lane >> 4 ) + 4 r = frame
#pragma unroll
			for( int r = 0; r < 4; r++ )
			{
				const int f = kq + 4 * r;
				if( bin0 == 0 )
				{
					t.pw[ f ][ 0 ] = re0[ r ] * re0[ r ];
					t.pw[ f ][ 128 ] = im0[ r ] * im0[ r ];
				}
				else t.pw[ f ][ bin0 ] = fma( re0[ r ], re0[ r ], im0[ r ] * im0[ r ] );
				t.pw[ f ][ bin1 ] = fma( re1[ r ], re1[ r ], im1[ r ] * im1[ r ] );
			}
		}
		__syncthreads();

		// ---- per frame: energy, the dominant bin, the two spectral sums. Wave w owns frames 4 w .. 4 w + 3 ----
		for( int j = 0; j < VAD_FR / VAD_WAVES; j++ )
		{
			const int f = wave * ( VAD_FR / VAD_WAVES ) + j;
			if( f < lo || f >= hi ) continue;	 // wave-uniform
			const float* const x = t.xs + f * VAD_X_STRIDE;
			double e = 0.0;
#pragma unroll
			for( int q = 0; q < 4; q++ )
			{
				const float v = x[ lane + 64 * q ];
				e += (double)__fmul_rn( v, v );
			}
			const double pa = t.pw[ f ][ lane ], pb = t.pw[ f ][ lane + 64 ];
			// bins 1 .. 127 stand for two of the 256, bins 0 and 128 for one
			const double wa = lane == 0 ? 1.0 : 2.0;
			double sumAbs = wa * sqrt( pa ) + 2.0 * sqrt( pb );
			double sumLn = wa * ( 0.5 * log( pa ) ) + 2.0 * ( 0.5 * log( pb ) );
			if( lane == 0 )
			{
				const double pn = t.pw[ f ][ 128 ];
				sumAbs += sqrt( pn );
				sumLn += 0.5 * log( pn );
			}
			// the first maximum of bins 0 .. 127: a strictly greater value, or an equal one at a lower bin, replaces
			double best = pa;
			int bestBin = lane;
			if( pb > pa ) { best = pb; bestBin = lane + 64; }
#pragma unroll
			for( int o = 32; o > 0; o >>= 1 )
			{
				e += __shfl_xor( e, o, 64 );
				sumAbs += __shfl_xor( sumAbs, o, 64 );
				sumLn += __shfl_xor( sumLn, o, 64 );
				const double ob = __shfl_xor( best, o, 64 );
				const int oi = __shfl_xor( bestBin, o, 64 );
				if( ob > best || ( ob == best && oi < bestBin ) ) { best = ob; bestBin = oi; }
			}
			if( lane == 0 )
			{
				float* const out = feat + ( outFrame0 + f ) * 3;
				out[ 0 ] = (float)sqrt( (double)(float)( e * ( 1.0 / VAD_N ) ) );
				out[ 1 ] = __fmul_rn( 62.5f, (float)bestBin );
				const float ratio = (float)( exp( sumLn * ( 1.0 / VAD_N ) ) / ( sumAbs * ( 1.0 / VAD_N ) ) );
				out[ 2 ] = __fmul_rn( -10.0f, (float)log10( (double)ratio ) );
			}
		}
	}
}	// namespace wh
