// Reductions over a workgroup and the (value, index) pair of the sampling kernels: shared by elementwise.hip and sample.hip (device code, one copy per unit).
#pragma once
#include "common.h"

namespace wh
{
	namespace
	{
		// ---- block reductions ------------------------------------------------------------------------------------
		template<int NW>
		__device__ __forceinline__ float blockMax( float v, float* sh )
		{
			v = waveReduceMax( v );
			const int w = threadIdx.x >> 6;
			if( ( threadIdx.x & 63 ) == 0 ) sh[ w ] = v;
			__syncthreads();
			float r = sh[ 0 ];
#pragma unroll
			for( int i = 1; i < NW; i++ ) r = fmaxf( r, sh[ i ] );
			__syncthreads();
			return r;
		}
		template<int NW>
		__device__ __forceinline__ double blockSumD( double v, double* sh )
		{
			v = waveReduceSumD( v );
			const int w = threadIdx.x >> 6;
			if( ( threadIdx.x & 63 ) == 0 ) sh[ w ] = v;
			__syncthreads();
			double r = sh[ 0 ];
#pragma unroll
			for( int i = 1; i < NW; i++ ) r += sh[ i ];
			__syncthreads();
			return r;
		}

		// ---- (value, index) pairs: the order every sampler ranks tokens by ----
		struct ArgMax
		{
			float v;
			int i;
		};
		__device__ __forceinline__ ArgMax better( ArgMax a, ArgMax b )
		{
			// larger value wins; equal values resolve to the lower index (the reference's partial_sort leaves ties unspecified)
			if( b.v > a.v || ( b.v == a.v && b.i < a.i ) ) return b;
			return a;
		}
		__device__ __forceinline__ ArgMax blockArgMax( ArgMax a, ArgMax* sh )
		{
#pragma unroll
			for( int o = 32; o > 0; o >>= 1 )
			{
				ArgMax b;
				b.v = __shfl_xor( a.v, o, 64 );
				b.i = __shfl_xor( a.i, o, 64 );
				a = better( a, b );
			}
			const int w = threadIdx.x >> 6;
			if( ( threadIdx.x & 63 ) == 0 ) sh[ w ] = a;
			__syncthreads();
			ArgMax r = sh[ 0 ];
			for( int i = 1; i < 16; i++ ) r = better( r, sh[ i ] );
			__syncthreads();
			return r;
		}
	}	// namespace
}	// namespace wh
