// The row quantizers of the INT8 encoder products ("INT8 encoder products"; the product itself is gemm_i8.hip).
//
// Format (restated in numpy by tests/encoder_i8_ref.py): symmetric int8 with one FP32 scale per row of K values,
//   amax = max |x| over the row's FP16 values,  s = amax / 127 (IEEE FP32 division; 1 for a row of zeros),
//   q = rint( x / s ) (IEEE FP32 division, to nearest even), clamped to [-127, 127]: -128 is never produced.
// Every rounding point is an operation of its own: two divisions and one v_rndne_f32, with nothing between them a compiler could contract (no multiply-add
// pair exists in the sequence, and HIP's FP32 division is the correctly rounded one unless a build asks for less; __fdiv_rn says so at the site).
//
// quantizeRowsI8<LPR, NC>: LPR lanes own a row and hold it in registers, NC 16-byte loads per lane, consecutive across the lanes, all requested before the first
//   use; the amax by log2( LPR ) xor-shuffles; 8 bytes stored per lane and chunk, again consecutive across the lanes; lane 0 of the row writes the scale. No
//   atomics, no scratch, no LDS. Two instances: 16 lanes per row for K <= 1024 (the products of d = 1024 and below: a wave takes 4 rows), a wave per row up to
//   K = 5120 (the MLP's hidden rows). Memory-bound: 2 K bytes read and K + 4 written per row.
// layerNormI8: the encoder's LayerNorm with this quantizer behind it, the FP16 row never stored. A wave per row forms the row with layerNormRows (common.h) --
//   the function launchLayerNorm's kernel calls, so the FP16 values are that kernel's bit for bit -- and keeps the f16x4 pieces it would have stored; amax,
//   scale and bytes follow as above, 4 bytes per lane and 256-column chunk.
#include "kernels.h"

namespace wh
{
	namespace
	{
		__device__ __forceinline__ float rowScaleI8( float amax ) { return amax > 0.0f ? __fdiv_rn( amax, 127.0f ) : 1.0f; }
		__device__ __forceinline__ unsigned quantOneI8( f16 x, float s )
		{
			const float r = fminf( fmaxf( rintf( __fdiv_rn( (float)x, s ) ), -127.0f ), 127.0f );
			return (unsigned)(int)r & 0xFFu;
		}

		template<int LPR, int NC>
		__global__ void __launch_bounds__( 256 ) quantizeRowsI8( const f16* __restrict__ x, long long ldx, int8_t* __restrict__ q, float* __restrict__ scale, int rows, int K )
		{
			const int sub = threadIdx.x % LPR;
			const int row = blockIdx.x * ( 256 / LPR ) + threadIdx.x / LPR;
			const int rowC = row < rows ? row : rows - 1;	   // the lanes of a row beyond the end load the last row and store nothing
			const int chunks = K >> 3;
			const f16* const src = x + (long long)rowC * ldx;
			f16x8 v[ NC ];
#pragma unroll
			for( int i = 0; i < NC; i++ )
			{
				const int c = i * LPR + sub;
				v[ i ] = *(const f16x8*)( src + ( c < chunks ? c : chunks - 1 ) * 8 );
			}
			float amax = 0.0f;
#pragma unroll
			for( int i = 0; i < NC; i++ )
				if( i * LPR + sub < chunks )
				{
#pragma unroll
					for( int e = 0; e < 8; e++ ) amax = fmaxf( amax, fabsf( (float)v[ i ][ e ] ) );
				}
#pragma unroll
			for( int o = LPR / 2; o > 0; o >>= 1 ) amax = fmaxf( amax, __shfl_xor( amax, o, 64 ) );
			const float s = rowScaleI8( amax );
			if( row >= rows ) return;
			int8_t* const dst = q + (long long)row * K;
#pragma unroll
			for( int i = 0; i < NC; i++ )
			{
				const int c = i * LPR + sub;
				if( c >= chunks ) continue;
				u32x2 pk = { 0u, 0u };
#pragma unroll
				for( int e = 0; e < 4; e++ )
				{
					pk[ 0 ] |= quantOneI8( v[ i ][ e ], s ) << ( 8 * e );
					pk[ 1 ] |= quantOneI8( v[ i ][ 4 + e ], s ) << ( 8 * e );
				}
				*(u32x2*)( dst + c * 8 ) = pk;
			}
			if( sub == 0 ) scale[ row ] = s;
		}

		template<int MAXC>
		__device__ __forceinline__ void layerNormRowI8( const float* __restrict__ xr, const float* __restrict__ w, const float* __restrict__ b, int8_t* __restrict__ dst,
			float* __restrict__ scale, int d, int lane )
		{
			// the pieces layerNormKernel would have stored: piece i = columns ( lane + 64 i ) * 4 .. + 3, so c >> 8 == i (lane * 4 < 256)
			f16x4 h[ MAXC ];
#pragma unroll
			for( int i = 0; i < MAXC; i++ ) h[ i ] = f16x4{ (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f };
			layerNormRows<MAXC, 1>( xr, 0, 1, w, b, d, lane, [ & ]( int, int c, f16x4 v )
			{
#pragma unroll
				for( int i = 0; i < MAXC; i++ )
					if( ( c >> 8 ) == i ) h[ i ] = v;
			} );
			float amax = 0.0f;
#pragma unroll
			for( int i = 0; i < MAXC; i++ )
#pragma unroll
				for( int e = 0; e < 4; e++ ) amax = fmaxf( amax, fabsf( (float)h[ i ][ e ] ) );	   // pieces beyond d are zeros
			amax = waveReduceMax( amax );
			const float s = rowScaleI8( amax );
#pragma unroll
			for( int i = 0; i < MAXC; i++ )
			{
				const int c = ( lane + 64 * i ) * 4;
				if( c >= d ) continue;
				unsigned pk = 0u;
#pragma unroll
				for( int e = 0; e < 4; e++ ) pk |= quantOneI8( h[ i ][ e ], s ) << ( 8 * e );
				*(unsigned*)( dst + c ) = pk;
			}
			if( lane == 0 ) *scale = s;
		}

		__global__ void __launch_bounds__( 256 ) layerNormI8( const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
			int8_t* __restrict__ q, float* __restrict__ scale, int rows, int d )
		{
			const int lane = threadIdx.x & 63;
			const int row = blockIdx.x * 4 + ( threadIdx.x >> 6 );
			if( row >= rows ) return;
			const float* const xr = x + (long long)row * d;
			int8_t* const dst = q + (long long)row * d;
			// the instances of layerNormKernel (elementwise.hip), chosen by the same thresholds
			if( d <= 256 * 4 )
				layerNormRowI8<4>( xr, w, b, dst, scale + row, d, lane );
			else if( d <= 256 * 5 )
				layerNormRowI8<5>( xr, w, b, dst, scale + row, d, lane );
			else
				layerNormRowI8<8>( xr, w, b, dst, scale + row, d, lane );
		}
	}	// namespace

	int launchQuantizeRowsI8( const f16* x, long long ldx, int8_t* q, float* scale, int rows, int K, hipStream_t stream )
	{
		if( !x || !q || !scale || rows <= 0 || K <= 0 || ( K % 128 ) != 0 || K > 5120 || ldx < K || ( ldx % 8 ) != 0 || ( (size_t)x % 16 ) != 0 || ( (size_t)q % 8 ) != 0 )
		{
			setError( "quantizeRowsI8: K must be a multiple of 128, at most 5120; rows at least K apart, 16-byte aligned" );
			return -1;
		}
		if( K <= 1024 )
			hipLaunchKernelGGL( ( quantizeRowsI8<16, 8> ), dim3( ( rows + 15 ) / 16 ), dim3( 256 ), 0, stream, x, ldx, q, scale, rows, K );
		else
			hipLaunchKernelGGL( ( quantizeRowsI8<64, 10> ), dim3( ( rows + 3 ) / 4 ), dim3( 256 ), 0, stream, x, ldx, q, scale, rows, K );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchLayerNormI8( const float* x, const float* w, const float* b, int8_t* q, float* scale, int rows, int d, hipStream_t stream )
	{
		if( !x || !w || !b || !q || !scale || rows <= 0 || ( d & 3 ) != 0 || d <= 0 || d > 2048 || ( (size_t)q % 4 ) != 0 )
		{
			setError( "layerNormI8: d must be a multiple of 4, at most 2048" );
			return -1;
		}
		hipLaunchKernelGGL( layerNormI8, dim3( ( rows + 3 ) / 4 ), dim3( 256 ), 0, stream, x, w, b, q, scale, rows, d );
		WH_HIP( hipGetLastError() );
		return 0;
	}
}
