// Normalisation, embedding and layout kernels (HBM-bound; LayerNorm one wave per row, shuffle reductions). The vocabulary-row kernels (softmax, samplers,
// language detection) are sample.hip's, the beam ranking and the cache reorder beam.hip's.
#include "kernels.h"

namespace wh
{
	namespace
	{
		// ---- LayerNorm + affine -> FP16 -----------------------------------------------------------------------------
		// norm.hlsl / normFixed.hlsl + fmaRepeat1.hlsl of the reference; numerics of ggml_compute_forward_norm_f32
		// (Whisper/source/ggml.c:4098-4156): mean, centred sum of squares, 1/sqrt(var + 1e-5), then w*y + b as two
		// separate FP32 operations (whisper.cpp:1195-1199), then the FP16 rounding the next weight product applies.
		// The reference sums in double; FP32 two-pass with a wavefront shuffle tree differs by ~1e-7 relative.
		constexpr int LN_MAX_CHUNKS = 8;	 // rows up to 2048 columns

		__global__ void __launch_bounds__( 256 ) layerNormKernel( const float* __restrict__ x, const float* __restrict__ w,
			const float* __restrict__ b, f16* __restrict__ out, int rows, int d )
		{
			const int lane = threadIdx.x & 63;
			const int row = blockIdx.x * 4 + ( threadIdx.x >> 6 );
			if( row >= rows ) return;
			f16* const o = out + (long long)row * d;
			// d <= 1280 for every Whisper size: the 5-chunk instance keeps the register count (and the wasted clamped loads) low
			if( d <= 256 * 4 )	  // (the medium shape: no fifth, clamped chunk -- a quarter more load instructions for nothing; same sums)
				layerNormRows<4, 1>( x + (long long)row * d, 0, 1, w, b, d, lane, [ = ]( int, int c, f16x4 v ) { *(f16x4*)( o + c ) = v; } );
			else if( d <= 256 * 5 )
				layerNormRows<5, 1>( x + (long long)row * d, 0, 1, w, b, d, lane, [ = ]( int, int c, f16x4 v ) { *(f16x4*)( o + c ) = v; } );
			else
				layerNormRows<LN_MAX_CHUNKS, 1>( x + (long long)row * d, 0, 1, w, b, d, lane, [ = ]( int, int c, f16x4 v ) { *(f16x4*)( o + c ) = v; } );
		}

		// ---- mel window -> padded FP16 conv input -----------------------------------------------------------------
		// MelInputTensor::create (Whisper/Whisper/MelInputTensor.cpp:8-63) + convolutionPrep1.hlsl: slice
		// [offset, offset + T) of each spectrogram, zero beyond its end, transposed to time-major and rounded to FP16
		// (the convolution rounds its input, ggml.c:5252-5287). Row 0 and row T+1 stay zero: the conv's zero padding.
		// `wins` non-null: every window names its own spectrogram (pointer, length, offset) -- the streams of a batch scheduler are
		// recordings of different lengths; a null pointer is a window of zeros.
		__global__ void __launch_bounds__( 256 ) melToConvInput( const float* __restrict__ mel, long long melStride, long long melLen,
			const int* __restrict__ melOffsets, const MelWindow* __restrict__ wins, f16* __restrict__ x16, long long xBatchStride, int nMels, int T )
		{
			__shared__ float tile[ 64 ][ 65 ];
			const int b = blockIdx.z;
			const int t0 = blockIdx.x * 64;
			const int c0 = blockIdx.y * 64;
			int off = melOffsets ? melOffsets[ b ] : 0;
			const float* src = mel + (long long)b * melStride;
			if( wins )
			{
				const MelWindow w = wins[ b ];
				src = w.mel;
				melLen = w.mel ? w.len : 0;
				off = w.offset;
			}
			const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
			for( int r = ty; r < 64; r += 4 )
			{
				const int c = c0 + r;
				const long long t = (long long)off + t0 + tx;
				float v = 0.0f;
				if( c < nMels && t0 + tx < T && t < melLen )
					v = src[ (long long)c * melLen + t ];
				tile[ r ][ tx ] = v;
			}
			__syncthreads();
			for( int r = ty; r < 64; r += 4 )
			{
				const int t = t0 + r;
				const int c = c0 + tx;
				if( t < T && c < nMels )
					x16[ (long long)b * xBatchStride + (long long)( t + 1 ) * nMels + c ] = (f16)tile[ tx ][ r ];
			}
		}

		// ---- token + position embedding (addRows.hlsl; whisper.cpp:1544-1548) ---------------------------------------
		__global__ void __launch_bounds__( 256 ) embedKernel( const int* __restrict__ tokens, const f16* __restrict__ te,
			const float* __restrict__ pe, float* __restrict__ x, int rows, int nTok, int nPast, const int* __restrict__ nPastDev, int d,
			int nVocab, int nTextCtx )
		{
			const int row = blockIdx.x;
			// ids and positions index two tables: both are clamped to the tables' extents, so that no value in tokensDev or in the
			// device-resident position can turn into an out-of-range read (the host entry points reject such ids before they get here)
			int tok = tokens[ row ];
			tok = tok < 0 ? 0 : ( tok >= nVocab ? nVocab - 1 : tok );
			int pos = ( nPastDev ? nPastDev[ row / nTok ] : nPast ) + row % nTok;
			pos = pos < 0 ? 0 : ( pos >= nTextCtx ? nTextCtx - 1 : pos );
			for( int c = threadIdx.x; c < d; c += 256 )
				x[ (long long)row * d + c ] = (float)te[ (long long)tok * d + c ] + pe[ (long long)pos * d + c ];
		}

		// ragged prompt step: the row of sequence b's last real token, lastPos[b], -> its row nTok - 1 (f16, d % 8 == 0)
		__global__ void __launch_bounds__( 256 ) gatherLastRowsKernel( f16* __restrict__ xn, const int* __restrict__ lastPos, int nTok, int d )
		{
			const int b = blockIdx.x;
			int last = lastPos[ b ];
			last = last < 0 ? 0 : ( last > nTok - 1 ? nTok - 1 : last );
			if( last == nTok - 1 ) return;
			const f16* const src = xn + ( (long long)b * nTok + last ) * d;
			f16* const dst = xn + ( (long long)b * nTok + nTok - 1 ) * d;
			for( int c = threadIdx.x * 8; c < d; c += 256 * 8 ) *(f16x8*)( dst + c ) = *(const f16x8*)( src + c );
		}
	}	// namespace

	int launchLayerNorm( const float* x, const float* w, const float* b, f16* out, int rows, int d, hipStream_t stream )
	{
		if( ( d & 3 ) != 0 || d > 256 * LN_MAX_CHUNKS || rows <= 0 )
		{
			setError( "layerNorm: d must be a multiple of 4, at most 2048" );
			return -1;
		}
		hipLaunchKernelGGL( layerNormKernel, dim3( ( rows + 3 ) / 4 ), dim3( 256 ), 0, stream, x, w, b, out, rows, d );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchMelToConvInput( const float* mel, long long melStride, long long melLen, const int* melOffsets, const MelWindow* wins, f16* x16,
		long long xBatchStride, int nMels, int T, int batch, hipStream_t stream )
	{
		dim3 grid( ( T + 63 ) / 64, ( nMels + 63 ) / 64, batch );
		hipLaunchKernelGGL( melToConvInput, grid, dim3( 256 ), 0, stream, mel, melStride, melLen, melOffsets, wins, x16, xBatchStride, nMels, T );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchEmbed( const int* tokens, const f16* te, const float* pe, float* x, int rows, int nTok, int nPast, const int* nPastDev, int d,
		int nVocab, int nTextCtx, hipStream_t stream )
	{
		hipLaunchKernelGGL( embedKernel, dim3( rows ), dim3( 256 ), 0, stream, tokens, te, pe, x, rows, nTok, nPast, nPastDev, d, nVocab, nTextCtx );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchGatherLastRows( f16* xn, const int* lastPos, int batch, int nTok, int d, hipStream_t stream )
	{
		if( ( d & 7 ) != 0 || batch <= 0 || nTok <= 0 ) { setError( "gatherLastRows: bad shape" ); return -1; }
		hipLaunchKernelGGL( gatherLastRowsKernel, dim3( batch ), dim3( 256 ), 0, stream, xn, lastPos, nTok, d );
		WH_HIP( hipGetLastError() );
		return 0;
	}
}
