// What the vocabulary-row kernels of sample.hip share, each piece stated once (device code, one copy per unit): reductions over a workgroup, the (value, index)
// pair tokens are ranked by, ContextImpl::sampleBest's rules on a row (Whisper/Whisper/ContextImpl.cpp:71-157: statistics, initial-timestamp cap, the top rounds,
// the TokenData record), the greedy loop's bookkeeping with the host mailbox, and the table softmax of a row held in registers.
#pragma once
#include "kernels.h"

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
		__device__ __forceinline__ ArgMax waveArgMax( ArgMax a )
		{
#pragma unroll
			for( int o = 32; o > 0; o >>= 1 )
			{
				ArgMax b;
				b.v = __shfl_xor( a.v, o, 64 );
				b.i = __shfl_xor( a.i, o, 64 );
				a = better( a, b );
			}
			return a;
		}
		template<int NW>
		__device__ __forceinline__ ArgMax blockArgMax( ArgMax a, ArgMax* sh )
		{
			a = waveArgMax( a );
			const int w = threadIdx.x >> 6;
			if( ( threadIdx.x & 63 ) == 0 ) sh[ w ] = a;
			__syncthreads();
			ArgMax r;
			// (four waves merge in pairs, more of them one after the other: with a NaN among the values the two orders can differ, and each keeps the one it had)
			if constexpr( NW == 4 )
				r = better( better( sh[ 0 ], sh[ 1 ] ), better( sh[ 2 ], sh[ 3 ] ) );
			else
			{
				r = sh[ 0 ];
				for( int i = 1; i < NW; i++ ) r = better( r, sh[ i ] );
			}
			__syncthreads();
			return r;
		}

		// ---- ContextImpl::sampleBest's rules on a row of probabilities ----
		// the first sample of a window may not pass 1.00 s: the timestamps behind it are masked (columns tsEnd .. nVocab)
		__device__ __forceinline__ int timestampEnd( int isInitial, int tokenBeg, int nVocab ) { return isInitial ? min( tokenBeg + 101, nVocab ) : nVocab; }
		__device__ __forceinline__ bool specialToken( int id, int tokenSot, int tokenSolm, int tokenNot ) { return id == tokenSot || id == tokenSolm || id == tokenNot; }

		// Best text token, best timestamp and the timestamps' mass. A kernel feeds every column of its own sweep (strided over memory or unrolled over registers),
		// thread by thread in column order, then reduces: the sum has the same bits wherever the sweep visits the same columns per thread.
		struct RowStats
		{
			ArgMax tx = { -1.0f, 0x7fffffff }, ts = { -1.0f, 0x7fffffff };
			double sumTs = 0.0;
			__device__ __forceinline__ void feed( float v, int c, int tokenBeg, int tsEnd )
			{
				if( c < tokenBeg )
					tx = better( tx, ArgMax{ v, c } );
				else if( c < tsEnd )
				{
					ts = better( ts, ArgMax{ v, c } );
					sumTs += (double)v;
				}
			}
			// 1024 threads; true = only timestamps may be sampled (their mass exceeds the best text token's probability, or the caller forces one)
			__device__ __forceinline__ bool reduce( int forceTimestamp, ArgMax* sha, double* shd )
			{
				tx = blockArgMax<16>( tx, sha );
				ts = blockArgMax<16>( ts, sha );
				sumTs = blockSumD<16>( sumTs, shd );
				return ( sumTs > (double)fmaxf( tx.v, -1.0f ) ) || forceTimestamp;
			}
		};

		// The best token of row p (memory, 1024 threads) from column lo on that the initial-timestamp cap does not mask and that is not among taken[ 0 .. nTaken )
		__device__ __forceinline__ ArgMax bestUntaken( const float* __restrict__ p, int lo, int nVocab, int tokenBeg, int tsEnd, const int* taken, int nTaken, ArgMax* sha )
		{
			ArgMax best = { -INFINITY, 0x7fffffff };
			for( int c = lo + threadIdx.x; c < nVocab; c += 1024 )
			{
				bool skip = c >= tsEnd && c >= tokenBeg;	  // masked by the initial-timestamp cap
				for( int k = 0; k < nTaken; k++ ) skip = skip || ( taken[ k ] == c );
				if( !skip ) best = better( best, ArgMax{ p[ c ], c } );
			}
			return blockArgMax<16>( best, sha );
		}
		// sampleBest's pick: the top 4 over the surviving tokens, the first one that is not sot / solm / not (the fourth whatever it is)
		__device__ __forceinline__ ArgMax sampleBestPick( const float* __restrict__ p, int nVocab, int tokenBeg, int tsEnd, bool onlyTs, int tokenSot, int tokenSolm,
			int tokenNot, ArgMax* sha )
		{
			const int lo = onlyTs ? tokenBeg : 0;
			int taken[ 4 ];
			ArgMax pick = { -INFINITY, 0 };
			for( int round = 0; round < 4; round++ )
			{
				pick = bestUntaken( p, lo, nVocab, tokenBeg, tsEnd, taken, round, sha );
				taken[ round ] = pick.i;
				if( !specialToken( pick.i, tokenSot, tokenSolm, tokenNot ) ) break;
			}
			return pick;
		}

		__device__ __forceinline__ TokenData sampleRecord( ArgMax pick, ArgMax ts, double sumTs, int nVocab )
		{
			// NaN logits compare false everywhere and would leave the sentinel index: never hand an out-of-range id to the
			// embedding gather of the next step
			if( pick.i < 0 || pick.i >= nVocab ) pick.i = 0;
			TokenData r;
			r.id = pick.i;
			r.tid = ts.v > -1.0f ? ts.i : 0;
			r.p = pick.v;
			r.pt = (float)( (double)ts.v / ( sumTs + 1e-10 ) );
			r.ptsum = (float)sumTs;
			return r;
		}

		// ---- the greedy loop's bookkeeping, by ONE thread of the row's workgroup: the sample's slot, the token the next step embeds, the host mailbox ----
		__device__ __forceinline__ void publishSample( const DecodeState* __restrict__ state, const SampleMailbox mail, TokenData* __restrict__ out,
			int* __restrict__ nextTokens, const TokenData r, int row, int rows )
		{
			const long long slot = (long long)state->step * rows + row;
			out[ slot ] = r;
			nextTokens[ row ] = r.id;
			const int gen = state->gen;
			if( mail.data && gen != 0 )
			{
				// host mailbox (pinned): the record as write-through stores, drained, then the stamp the host polls. No release
				// fence: at system scope that is a write-back of the whole L2 (measured +32 us per step at 112 rows); the order
				// data -> stamp is kept by waiting for the data stores before the stamp is issued (MI355X_MICROARCH.md, handoff-flag)
				int* const md = (int*)( mail.data + slot );
				__hip_atomic_store( md + 0, r.id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
				__hip_atomic_store( md + 1, r.tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
				__hip_atomic_store( md + 2, __float_as_int( r.p ), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
				__hip_atomic_store( md + 3, __float_as_int( r.pt ), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
				__hip_atomic_store( md + 4, __float_as_int( r.ptsum ), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
				// the record validates itself: a word that depends on every field and on the generation travels with it, so a host that
				// ever saw the stamp before all of the record (the order below rests on store acknowledgements, not on a release) reads a
				// checksum that does not match and keeps polling instead of consuming a torn record
				__hip_atomic_store( mail.flag + 2 * slot + 1, sampleChecksum( gen, r ), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
				asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
				__hip_atomic_store( mail.flag + 2 * slot, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
			}
		}

		// ---- table softmax with the ROW IN REGISTERS (1024 threads, cols <= PER * 1024) ----
		// SCALED (temperature sampling, wh_op_vocab_soft_max_scaled): the row is x * invT, each product rounded once to FP32 (__fmul_rn: never contracted into the
		// subtraction of the maximum). The unscaled instances ignore invT and compile to the code they had before the parameter existed.
		template<bool SCALED>
		__device__ __forceinline__ float softMaxInput( float x, float invT )
		{
			if constexpr( SCALED ) return __fmul_rn( x, invT );
			else return x;
		}
		// Column threadIdx.x + 1024 * i of row x -> v[ i ], -inf beyond the row's end; returns the thread's maximum
		template<int PER, bool SCALED>
		__device__ __forceinline__ float loadRowReg( const float* __restrict__ x, int cols, float invT, float ( &v )[ PER ] )
		{
			float m = -INFINITY;
#pragma unroll
			for( int i = 0; i < PER; i++ )
			{
				const int c = threadIdx.x + 1024 * i;
				const float t = softMaxInput<SCALED>( x[ c < cols ? c : cols - 1 ], invT );	  // (clamped address + select: a branch per element would serialise the loads)
				v[ i ] = c < cols ? t : -INFINITY;
				m = fmaxf( m, v[ i ] );
			}
			return m;
		}
		// m = the thread's maximum of its v[]; v[ i ] -> e = exp16( v[ i ] - row maximum ) in place (0 at -inf); inv = float( 1 / sum ), the sum in double thread by thread in column order: p = e * inv has
		// softMaxRows' bits.
		struct RowNorm { float max, inv; };
		template<int PER>
		__device__ __forceinline__ RowNorm softMaxRowReg( float ( &v )[ PER ], float m, float* shf, double* shd )
		{
			m = blockMax<16>( m, shf );
			double s = 0.0;
#pragma unroll
			for( int i = 0; i < PER; i++ )
			{
				const float e = ( v[ i ] == -INFINITY ) ? 0.0f : exp16( v[ i ] - m );
				v[ i ] = e;
				s += (double)e;
			}
			s = blockSumD<16>( s, shd );
			return RowNorm{ m, (float)( 1.0 / s ) };
		}
	}	// namespace
}	// namespace wh
