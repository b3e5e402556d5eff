// ggml's block-quantized weights -> FP16 on the GPU (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 of quantization version 2): what the model loader runs on every
// quantized matrix of a file, once, at load time (wh_model_set_tensor). Nothing on the timed path reads a block.
//
// A block is 32 consecutive elements of a row: an FP16 scale d, for the _1 types an FP16 offset m, for the 5-bit types the 32 fifth bits qh, then the
// quants qs. Element i of the block is
//   Q4_0 / Q5_0 / Q8_0   w = fp16_rne( (float)d * (float)( q - off ) )        off = 8, 16, 0
//   Q4_1 / Q5_1          w = fp16_rne( (float)d * (float)q + (float)m )
// with q of element j < 16 the low nibble of qs[ j ], of element j + 16 the high nibble (plus bit j, j + 16 of qh << 4); Q8_0: q = (int8)qs[ i ].
// d and q - off have at most 11 and 8 significant bits: the product is exact in FP32, so for the _0 types it equals the FP16 product of d and the FP16 number
// q - off (one rounding either way), and for the _1 types a contracted multiply-add and a separate one give the same sum, which is rounded once to FP32 and
// then to FP16. Overflow gives +-inf, a NaN scale NaN, FP16 subnormals are read and written as such.
//
// Kernel: streaming. Blocks are 18 .. 34 bytes with no padding, so a block is only 2-byte aligned and no lane may read one with a wide load. A workgroup
// owns DQ_SPAN = 256 blocks: 256 x blockBytes is a multiple of 16 for every type, so with a 16-byte aligned source every span starts 16-byte aligned and is
// copied to LDS with dwordx4 loads, consecutive across lanes (the last span's remainder, less than 16 bytes, with 2-byte loads: nothing behind the source is
// read). Then lane t of pass p produces the 8 consecutive outputs 8 ( 256 p + t ) .. + 7 of the span -- a quarter of a block, whose 8 quants are 8 (Q8_0) or
// the low or high nibbles of 8 (Q4, Q5) consecutive bytes of qs, read from LDS as 16-bit words -- and stores them with one 16-byte store: a wave instruction
// writes 1 KB without a gap. No atomics, no cross-lane traffic; a lane whose block lies behind nBlocks neither reads LDS nor stores.
#include "runtime.h"

namespace wh
{
	namespace
	{
		constexpr int DQ_THREADS = 256, DQ_SPAN = 256;
		constexpr int DQ_MAX_BLOCK_BYTES = 34;
		static_assert( ( DQ_SPAN % 8 ) == 0, "a span of every block size must be a multiple of 16 bytes" );
		static_assert( ( DQ_SPAN * 4 ) % DQ_THREADS == 0, "four lanes per block, whole passes" );

		// ggml type numbers
		enum { T_Q4_0 = 2, T_Q4_1 = 3, T_Q5_0 = 6, T_Q5_1 = 7, T_Q8_0 = 8 };

		template<int TYPE> struct BlockTraits;
		template<> struct BlockTraits<T_Q4_0> { static constexpr int bytes = 18, qh = -1, qs = 2, off = 8; static constexpr bool hasM = false; };
		template<> struct BlockTraits<T_Q4_1> { static constexpr int bytes = 20, qh = -1, qs = 4, off = 0; static constexpr bool hasM = true; };
		template<> struct BlockTraits<T_Q5_0> { static constexpr int bytes = 22, qh = 2, qs = 6, off = 16; static constexpr bool hasM = false; };
		template<> struct BlockTraits<T_Q5_1> { static constexpr int bytes = 24, qh = 4, qs = 8, off = 0; static constexpr bool hasM = true; };
		template<> struct BlockTraits<T_Q8_0> { static constexpr int bytes = 34, qh = -1, qs = 2, off = 0; static constexpr bool hasM = false; };

		__device__ inline float halfBits( unsigned short u )
		{
			return (float)__builtin_bit_cast( _Float16, u );
		}

		template<int TYPE>
		__global__ void __launch_bounds__( DQ_THREADS ) dequantKernel( const uint4* __restrict__ src, long long nBlocks, f16x8* __restrict__ dst )
		{
			typedef BlockTraits<TYPE> B;
			constexpr int SPAN_BYTES = DQ_SPAN * B::bytes;
			__shared__ uint4 stage[ DQ_SPAN * DQ_MAX_BLOCK_BYTES / 16 ];

			const int tid = threadIdx.x;
			const long long block0 = (long long)blockIdx.x * DQ_SPAN;
			const long long left = nBlocks - block0;
			const int here = left < DQ_SPAN ? (int)left : DQ_SPAN;	  // blocks of this span: 1 .. DQ_SPAN
			const int bytes = here * B::bytes;
			{
				const uint4* const g = src + (long long)blockIdx.x * ( SPAN_BYTES / 16 );
				const int full = bytes >> 4;
				for( int i = tid; i < full; i += DQ_THREADS ) stage[ i ] = g[ i ];
				// the remainder of the last span: 2 .. 14 bytes
				const unsigned short* const g2 = (const unsigned short*)g;
				unsigned short* const s2 = (unsigned short*)stage;
				for( int i = ( full << 3 ) + tid; i < ( bytes >> 1 ); i += DQ_THREADS ) s2[ i ] = g2[ i ];
			}
			__syncthreads();

			const unsigned short* const words = (const unsigned short*)stage;
#pragma unroll
			for( int pass = 0; pass < DQ_SPAN * 4 / DQ_THREADS; pass++ )
			{
				const int group = pass * DQ_THREADS + tid;	  // 8 outputs
				const int blk = group >> 2, quarter = group & 3;
				if( blk >= here ) break;
				const unsigned short* const b = words + blk * ( B::bytes / 2 );
				const _Float16 dh = __builtin_bit_cast( _Float16, b[ 0 ] );
				const float d = (float)dh;
				const float m = B::hasM ? halfBits( b[ 1 ] ) : 0.0f;
				int q[ 8 ];
				if( TYPE == T_Q8_0 )
				{
#pragma unroll
					for( int i = 0; i < 4; i++ )
					{
						const unsigned w = b[ B::qs / 2 + quarter * 4 + i ];
						q[ 2 * i ] = (int)(signed char)( w & 0xFF );
						q[ 2 * i + 1 ] = (int)(signed char)( w >> 8 );
					}
				}
				else
				{
					// elements 8 quarter .. + 7: bytes 8 ( quarter & 1 ) .. + 7 of qs, the low nibbles for quarters 0 and 1, the high ones for 2 and 3
					const int shift = ( quarter >> 1 ) * 4;
					unsigned fifth = 0;
					if( B::qh >= 0 )
					{
						const unsigned qh = (unsigned)b[ B::qh / 2 ] | ( (unsigned)b[ B::qh / 2 + 1 ] << 16 );
						fifth = qh >> ( quarter * 8 );	  // bit i = the fifth bit of element 8 quarter + i
					}
#pragma unroll
					for( int i = 0; i < 4; i++ )
					{
						const unsigned w = b[ B::qs / 2 + ( quarter & 1 ) * 4 + i ];
						q[ 2 * i ] = (int)( ( w >> shift ) & 15 );
						q[ 2 * i + 1 ] = (int)( ( w >> ( 8 + shift ) ) & 15 );
					}
					if( B::qh >= 0 )
					{
#pragma unroll
						for( int i = 0; i < 8; i++ ) q[ i ] |= (int)( ( fifth >> i ) & 1 ) << 4;
					}
				}
				f16x8 out;
#pragma unroll
				for( int i = 0; i < 8; i++ )
				{
					if( B::hasM )
						out[ i ] = (_Float16)( d * (float)q[ i ] + m );
					else
					{
						// The FP32 product of two FP16 numbers is exact, so rounding it to FP16 IS the FP16 product: written as such. As
						// (_Float16)( d * v ) two of the eight came out as v_fma_mix( d, v, +0 ), which turns the -0 of a negative d times q == off into +0.
						out[ i ] = dh * (_Float16)( q[ i ] - B::off );
					}
				}
				dst[ ( block0 << 2 ) + group ] = out;
			}
		}

		template<int TYPE>
		int launchOne( hipStream_t stream, const void* src, long long nBlocks, void* dst )
		{
			const long long spans = ( nBlocks + DQ_SPAN - 1 ) / DQ_SPAN;
			hipLaunchKernelGGL( dequantKernel<TYPE>, dim3( (unsigned)spans ), dim3( DQ_THREADS ), 0, stream, (const uint4*)src, nBlocks, (f16x8*)dst );
			WH_HIP( hipGetLastError() );
			return 0;
		}
	}	// namespace

	int dequantBlockBytes( int type )
	{
		switch( type )
		{
		case T_Q4_0: return BlockTraits<T_Q4_0>::bytes;
		case T_Q4_1: return BlockTraits<T_Q4_1>::bytes;
		case T_Q5_0: return BlockTraits<T_Q5_0>::bytes;
		case T_Q5_1: return BlockTraits<T_Q5_1>::bytes;
		case T_Q8_0: return BlockTraits<T_Q8_0>::bytes;
		default: return 0;
		}
	}

	int launchDequantize( hipStream_t stream, int type, const void* src, long long nBlocks, void* dst )
	{
		if( nBlocks <= 0 ) return 0;
		switch( type )
		{
		case T_Q4_0: return launchOne<T_Q4_0>( stream, src, nBlocks, dst );
		case T_Q4_1: return launchOne<T_Q4_1>( stream, src, nBlocks, dst );
		case T_Q5_0: return launchOne<T_Q5_0>( stream, src, nBlocks, dst );
		case T_Q5_1: return launchOne<T_Q5_1>( stream, src, nBlocks, dst );
		case T_Q8_0: return launchOne<T_Q8_0>( stream, src, nBlocks, dst );
		default: setError( "dequantize: not a quantized type" ); return WH_E_INVALIDARG;
		}
	}
}	// namespace wh

extern "C" {

int wh_dequantize( void* stream, int type, const void* srcDev, int64_t nBlocks, void* dstDev )
{
	if( dequantBlockBytes( type ) == 0 )
	{
		setError( "dequantize: type " + std::to_string( type ) + " is not one of 2 (q4_0), 3 (q4_1), 6 (q5_0), 7 (q5_1), 8 (q8_0)" );
		return WH_E_INVALIDARG;
	}
	if( nBlocks < 0 || nBlocks > 0x7FFFFFFF ) { setError( "dequantize: nBlocks 0 .. 2^31 - 1 blocks of 32" ); return WH_E_INVALIDARG; }
	if( nBlocks == 0 ) return 0;
	if( !srcDev || !dstDev || ( (uintptr_t)srcDev & 15 ) != 0 || ( (uintptr_t)dstDev & 15 ) != 0 )
	{
		setError( "dequantize: null buffer, or one that is not 16-byte aligned" );
		return WH_E_INVALIDARG;
	}
	return launchDequantize( (hipStream_t)stream, type, srcDev, nBlocks, dstDev );
}

}	// extern "C"
