// The vocabulary-row kernels: table softmax, ContextImpl::sampleBest on the device (alone, fused behind the softmax, spread over the chip, as beam candidates),
// language detection, and temperature sampling -- one categorical draw per row under sampleBest's own masks ("Decoding fallback"; the
// reference has no temperature anywhere: those rules are this project's and are restated in float64 by tests/fallback_ref.py). One 1024-thread workgroup per row
// unless a kernel says otherwise. What the kernels share -- sampleBest's rules, the record, the host mailbox -- is sampler_device.h's.
#include "kernels.h"
#include "sampler_device.h"

namespace wh
{
	namespace
	{
		// ---- table softmax over rows (softMax.hlsl / softMaxLong.hlsl; ggml.c:5030-5090) ---------------------------
		// p = exp16( x - max ) / sum, sum in double like the reference, -inf -> 0. One 1024-thread block per row.
		// SCALED: the row is softMaxInput's x * invT, invT by value or, when invTDev is non-null, read from device memory (a captured step graph outlives a change
		// of temperature). PER_ROW: invTDev is the head of an array of SampleRowParams records and row r takes its own record's factor.
		constexpr int ROW_PARAMS_STRIDE = (int)( sizeof( SampleRowParams ) / sizeof( float ) );
		static_assert( sizeof( SampleRowParams ) % sizeof( float ) == 0 && offsetof( SampleRowParams, invT ) == 0, "the softmax reads the factor at the head of each record" );
		template<bool SCALED, bool PER_ROW = false>
		__global__ void __launch_bounds__( 1024 ) softMaxRows( const float* in, float* out, int cols, float invT, const float* invTDev )
		{
			__shared__ float shf[ 16 ];
			__shared__ double shd[ 16 ];
			const float* x = in + (long long)blockIdx.x * cols;
			float* y = out + (long long)blockIdx.x * cols;
			if constexpr( PER_ROW ) invT = invTDev[ blockIdx.x * ROW_PARAMS_STRIDE ];
			else if constexpr( SCALED )
				if( invTDev ) invT = *invTDev;
			float m = -INFINITY;
			for( int c = threadIdx.x; c < cols; c += 1024 ) m = fmaxf( m, softMaxInput<SCALED>( x[ c ], invT ) );
			m = blockMax<16>( m, shf );
			double s = 0.0;
			for( int c = threadIdx.x; c < cols; c += 1024 )
			{
				const float v = softMaxInput<SCALED>( x[ c ], invT );
				const float e = ( v == -INFINITY ) ? 0.0f : exp16( v - m );
				y[ c ] = e;
				s += (double)e;
			}
			s = blockSumD<16>( s, shd );
			const float inv = (float)( 1.0 / s );
			for( int c = threadIdx.x; c < cols; c += 1024 ) y[ c ] = y[ c ] * inv;
		}

		// ---- ContextImpl::sampleBest on the device (Whisper/Whisper/ContextImpl.cpp:71-157) -------------------------
		__global__ void __launch_bounds__( 1024 ) sampleBestKernel( const float* __restrict__ probs, int nVocab, int tokenBeg,
			int tokenSot, int tokenSolm, int tokenNot, int forceTimestamp, int isInitial, TokenData* __restrict__ out )
		{
			__shared__ ArgMax sha[ 16 ];
			__shared__ double shd[ 16 ];
			const float* p = probs + (long long)blockIdx.x * nVocab;
			const int tsEnd = timestampEnd( isInitial, tokenBeg, nVocab );
			RowStats st;
			for( int c = threadIdx.x; c < nVocab; c += 1024 ) st.feed( p[ c ], c, tokenBeg, tsEnd );
			const bool onlyTs = st.reduce( forceTimestamp, sha, shd );
			const ArgMax pick = sampleBestPick( p, nVocab, tokenBeg, tsEnd, onlyTs, tokenSot, tokenSolm, tokenNot, sha );
			if( threadIdx.x == 0 ) out[ blockIdx.x ] = sampleRecord( pick, st.ts, st.sumTs, nVocab );
		}
		// ---- the `width` best continuations of a sequence under sampleBest's own rules (beam search on hypothesis groups) ----
		// Candidate 0 IS ContextImpl::sampleBest's pick (timestamp-vs-text sum rule, initial-timestamp cap, the top tokens that are
		// sot / solm / not skipped); candidates 1 .. width-1 are the next best tokens under the same mask, specials skipped as well.
		// So a beam of width 1 is the greedy decoder. out: [sequences][width] TokenData (tid / pt / ptsum repeated).
		__global__ void __launch_bounds__( 1024 ) beamCandidatesKernel( const float* __restrict__ probs, int nVocab, int tokenBeg,
			int tokenSot, int tokenSolm, int tokenNot, int forceTimestamp, int isInitial, int width, TokenData* __restrict__ out )
		{
			__shared__ ArgMax sha[ 16 ];
			__shared__ double shd[ 16 ];
			const float* p = probs + (long long)blockIdx.x * nVocab;
			const int tsEnd = timestampEnd( isInitial, tokenBeg, nVocab );
			RowStats st;
			for( int c = threadIdx.x; c < nVocab; c += 1024 ) st.feed( p[ c ], c, tokenBeg, tsEnd );
			const bool onlyTs = st.reduce( forceTimestamp, sha, shd );
			const int lo = onlyTs ? tokenBeg : 0;
			constexpr int MAXW = 8;
			int taken[ MAXW + 3 ];
			int nTaken = 0, found = 0;
			// at most width + 3 rounds: the three specials may each cost one
			for( int round = 0; round < width + 3 && found < width; round++ )
			{
				const ArgMax best = bestUntaken( p, lo, nVocab, tokenBeg, tsEnd, taken, nTaken, sha );
				// no token left under the mask (fewer than `width` survive): the rest repeats the last candidate with probability 0 below, not the
				// sentinel's token 0 at -inf (candidate 0 of an empty row keeps sampleBest's own answer)
				if( found > 0 && ( best.i < 0 || best.i >= nVocab ) ) break;
				taken[ nTaken++ ] = best.i;
				// sampleBest gives up after four rounds and takes the fourth token whatever it is: only candidate 0 can meet that rule
				if( specialToken( best.i, tokenSot, tokenSolm, tokenNot ) && !( found == 0 && round == 3 ) ) continue;
				if( threadIdx.x == 0 ) out[ (long long)blockIdx.x * width + found ] = sampleRecord( best, st.ts, st.sumTs, nVocab );
				found++;
			}
			// fewer than `width` tokens under the mask (cannot happen with a real vocabulary): repeat the last one with probability 0
			for( ; found < width; found++ )
				if( threadIdx.x == 0 )
				{
					TokenData r = out[ (long long)blockIdx.x * width + ( found > 0 ? found - 1 : 0 ) ];
					r.p = 0.0f;
					out[ (long long)blockIdx.x * width + found ] = r;
				}
		}

		// softMaxRows with the ROW IN REGISTERS (round 6, option beam_regs): one read and one write of the row instead of three reads and two writes (a workgroup per row:
		// 40 CUs at 40 rows) -- 37.8 -> 18.3 us at 40 x 51865. The same arithmetic in the same order (e = exp16( x - max ), the double sum thread by thread in column
		// order, p = e * float( 1 / sum )): the same bits. cols <= SC_PER * 1024. Built, measured and NOT kept: the candidate search the same way (51 selects per round and
		// thread where beamCandidatesKernel re-reads the row: 57.6 against 26 us, VALU-bound, a third of the row spilled), and both in one launch (124 us: 288 spill
		// instructions under the 128-register cap of a 1024-thread workgroup).
		constexpr int SC_PER = 51;
		template<bool SCALED, bool PER_ROW = false>
		__global__ void __launch_bounds__( 1024 ) softMaxRowsReg( const float* __restrict__ in, float* __restrict__ out, int cols, float invT, const float* __restrict__ invTDev )
		{
			__shared__ float shf[ 16 ];
			__shared__ double shd[ 16 ];
			const float* const x = in + (long long)blockIdx.x * cols;
			float* const y = out + (long long)blockIdx.x * cols;
			if constexpr( PER_ROW ) invT = invTDev[ blockIdx.x * ROW_PARAMS_STRIDE ];
			else if constexpr( SCALED )
				if( invTDev ) invT = *invTDev;
			float v[ SC_PER ];
			const float m = loadRowReg<SC_PER, SCALED>( x, cols, invT, v );
			const float inv = softMaxRowReg( v, m, shf, shd ).inv;
	#pragma unroll
			for( int i = 0; i < SC_PER; i++ )
			{
				const int c = threadIdx.x + 1024 * i;
				if( c < cols ) y[ c ] = v[ i ] * inv;
			}
		}
		// ---- language detection: the vocabulary softmax's statistics, only the language columns written (whisper.cpp:2428-2495) ----
		// Row r of the logits stands rowStride floats behind row r - 1 (the first sequence of every hypothesis group). The row maximum, e = exp16( x - max ) and the
		// double sum thread by thread in column order are softMaxRows' / softMaxRowsReg's, so p = e * float( 1 / sum ) at columns tokenSot + 1 .. tokenSot + nLang has
		// the same bits as what those kernels write there; the 51865-float row of probabilities is never written. best = the language with the largest p, exact
		// ties to the lower id. The row stays in registers between the two sweeps like softMaxRowsReg's (cols <= SC_PER * 1024; 124 VGPRs, no scratch). Reading it
		// twice instead (46 VGPRs) was built and measured: 30.9 / 53.2 us at 64 / 448 rows x 51865 against 18.0 / 36.8 us for this one -- not kept. nLang <= 1024.
		__global__ void __launch_bounds__( 1024 ) langProbsKernel( const float* __restrict__ in, long long rowStride, int cols, int tokenSot, int nLang,
			float* __restrict__ langP, int* __restrict__ best )
		{
			__shared__ float shf[ 16 ];
			__shared__ double shd[ 16 ];
			__shared__ ArgMax sha[ 16 ];
			const float* const x = in + (long long)blockIdx.x * rowStride;
			float v[ SC_PER ];
			const float m = loadRowReg<SC_PER, false>( x, cols, 1.0f, v );
			const RowNorm n = softMaxRowReg( v, m, shf, shd );
			// the language block is at most 1024 columns: thread t owns language t (the few logits are read once more, from the cache)
			ArgMax a = { -1.0f, 0x7fffffff };
			if( (int)threadIdx.x < nLang )
			{
				const float x1 = x[ tokenSot + 1 + threadIdx.x ];
				const float e = ( x1 == -INFINITY ) ? 0.0f : exp16( x1 - n.max );
				a.v = e * n.inv;
				a.i = threadIdx.x;
				langP[ (long long)blockIdx.x * nLang + threadIdx.x ] = a.v;
			}
			a = blockArgMax<16>( a, sha );
			if( threadIdx.x == 0 ) best[ blockIdx.x ] = ( a.i < 0 || a.i >= nLang ) ? 0 : a.i;	  // (NaN compares false everywhere and leaves the sentinel)
		}

		// The same two outputs from probabilities that exist already (WH_FLAG_PARITY_EXACT: the reference's own bits, exact.hip): a gather and an argmax.
		__global__ void __launch_bounds__( 1024 ) langGatherKernel( const float* __restrict__ probs, long long rowStride, int tokenSot, int nLang,
			float* __restrict__ langP, int* __restrict__ best )
		{
			__shared__ ArgMax sha[ 16 ];
			const float* const p = probs + (long long)blockIdx.x * rowStride;
			ArgMax a = { -1.0f, 0x7fffffff };
			if( (int)threadIdx.x < nLang )
			{
				a.v = p[ tokenSot + 1 + threadIdx.x ];
				a.i = threadIdx.x;
				langP[ (long long)blockIdx.x * nLang + threadIdx.x ] = a.v;
			}
			a = blockArgMax<16>( a, sha );
			if( threadIdx.x == 0 ) best[ blockIdx.x ] = ( a.i < 0 || a.i >= nLang ) ? 0 : a.i;
		}

		// ---- the score of a GIVEN token under a row of logits (wh_score_tokens; DESIGN.md section 7 "Scoring", restated in float64 by tests/token_score_ref.py) ----
		// Per row and target t: the row maximum m and the lowest id that has it, s = sum exp( x - m ) in double (FP32 expf per term, -inf adds 0), and
		// rank = #{ x[ j ] > x[ t ] } + #{ j < t : x[ j ] == x[ t ] }; logprob = x[ t ] - m - ln s and bestLogprob = -ln s in double, rounded once. True logarithms:
		// nothing of the FP16 exp table, whose e is 0 for an unlikely token. REG: the row in registers between the two sweeps like langProbsKernel's (one read with
		// consecutive lanes on consecutive floats, cols <= SC_PER * 1024); otherwise the row is read twice. Either way thread t visits columns t, t + 1024, ... in
		// that order and the three reductions are the same code, so the two forms give the same bits. 16 bytes written per row.
		struct ScoreAcc
		{
			double s = 0.0;
			int rank = 0, best = 0x7fffffff;
			__device__ __forceinline__ void feed( float v, int c, float m, float xt, int t )
			{
				s += ( v == -INFINITY ) ? 0.0 : (double)expf( v - m );
				rank += ( v > xt || ( v == xt && c < t ) ) ? 1 : 0;
				best = ( v == m && c < best ) ? c : best;
			}
		};
		template<bool REG>
		__global__ void __launch_bounds__( 1024 ) tokenScoreKernel( const float* __restrict__ in, long long rowStride, int cols, const int* __restrict__ targets,
			TokenScore* __restrict__ out )
		{
			__shared__ float shf[ 16 ];
			__shared__ double shd[ 16 ];
			__shared__ int shRank[ 16 ], shBest[ 16 ];
			const float* const x = in + (long long)blockIdx.x * rowStride;
			// (the entry points have checked the targets on the host; an id read from device memory is clamped into the row all the same)
			const int t = min( max( targets[ blockIdx.x ], 0 ), cols - 1 );
			const float xt = x[ t ];	 // a broadcast load
			ScoreAcc a;
			float m;
			if constexpr( REG )
			{
				float v[ SC_PER ];
				m = blockMax<16>( loadRowReg<SC_PER, false>( x, cols, 1.0f, v ), shf );
	#pragma unroll
				for( int i = 0; i < SC_PER; i++ ) a.feed( v[ i ], threadIdx.x + 1024 * i, m, xt, t );	  // (-inf beyond the row's end: adds 0, outranks nothing, never the maximum)
			}
			else
			{
				m = -INFINITY;
				for( int c = threadIdx.x; c < cols; c += 1024 ) m = fmaxf( m, x[ c ] );
				m = blockMax<16>( m, shf );
				for( int c = threadIdx.x; c < cols; c += 1024 ) a.feed( x[ c ], c, m, xt, t );
			}
			// the three reductions behind one barrier; the sum wave by wave in blockSumD's order
			a.s = waveReduceSumD( a.s );
	#pragma unroll
			for( int o = 32; o > 0; o >>= 1 )
			{
				a.rank += __shfl_xor( a.rank, o, 64 );
				a.best = min( a.best, __shfl_xor( a.best, o, 64 ) );
			}
			if( ( threadIdx.x & 63 ) == 0 )
			{
				const int w = threadIdx.x >> 6;
				shd[ w ] = a.s; shRank[ w ] = a.rank; shBest[ w ] = a.best;
			}
			__syncthreads();
			if( threadIdx.x == 0 )
			{
				double s = shd[ 0 ];
				int rank = shRank[ 0 ], best = shBest[ 0 ];
				for( int i = 1; i < 16; i++ )
				{
					s += shd[ i ];
					rank += shRank[ i ];
					best = min( best, shBest[ i ] );
				}
				const double lnS = log( s );
				TokenScore r;
				r.logprob = (float)( ( (double)xt - (double)m ) - lnS );
				r.bestLogprob = (float)( -lnS );
				r.best = ( best < 0 || best >= cols ) ? 0 : best;	  // (NaN compares false everywhere and leaves the sentinel)
				r.rank = rank;
				out[ blockIdx.x ] = r;
			}
		}

		// wh_score_tokens: the rows of the normalised decoder activations that predict a scored token, gathered compactly, and the tokens they are scored against.
		// Window b's rows first[ b ] - 1 .. len[ b ] - 2 of x [windows][nMax][d] go to rows off[ b ] .. of dst; targets[ that row ] = tokens[ b ][ i + 1 ].
		// meta: [ first | len | off ] x windows. One workgroup per (row i, window b), 16 bytes per thread and trip; d % 8 == 0.
		__global__ void __launch_bounds__( 128 ) gatherScoreRowsKernel( const f16* __restrict__ x, const int* __restrict__ tokens, const int* __restrict__ meta, int windows,
			int nMax, int d, f16* __restrict__ dst, int* __restrict__ targets )
		{
			const int b = blockIdx.y, i = blockIdx.x;
			const int first = meta[ b ], len = meta[ windows + b ], off = meta[ 2 * windows + b ];
			if( i < first - 1 || i > len - 2 ) return;
			const long long src = (long long)b * nMax + i, row = (long long)off + ( i - ( first - 1 ) );
			const uint4* const s = (const uint4*)( x + src * d );
			uint4* const o = (uint4*)( dst + row * d );
			for( int k = threadIdx.x; k < d / 8; k += 128 ) o[ k ] = s[ k ];
			if( threadIdx.x == 0 ) targets[ row ] = tokens[ src + 1 ];
		}

		// ---- logits row -> table softmax -> sampleBest in ONE kernel, the row held in registers -----------------------
		// Used by the captured decode step: no host round trip between the logits product and the next token. Same
		// arithmetic as softMaxRows followed by sampleBestKernel (p = exp16(x - max) * float(1 / double sum)).
		__global__ void __launch_bounds__( 1024 ) softMaxSampleKernel( const float* __restrict__ logits, float* __restrict__ probsOut,
			int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot, const DecodeState* __restrict__ state,
			TokenData* __restrict__ out, int* __restrict__ nextTokens, const SampleMailbox mail )
		{
			__shared__ float shf[ 16 ];
			__shared__ double shd[ 16 ];
			__shared__ ArgMax sha[ 16 ];
			const float* x = logits + (long long)blockIdx.x * nVocab;
			const int forceTimestamp = state->forceTimestamp, isInitial = state->isInitial;
			const int tsEnd = timestampEnd( isInitial, tokenBeg, nVocab );
			float v[ SC_PER ];
			// (a branch per element, not loadRowReg's clamped address: under this kernel's register pressure the compiler then waits for each load of the clamped
			// form before it issues the next -- 51 round trips, +9 us per token at the one row of a single stream, measured)
			float m = -INFINITY;
#pragma unroll
			for( int j = 0; j < SC_PER; j++ )
			{
				const int c = threadIdx.x + j * 1024;
				v[ j ] = c < nVocab ? x[ c ] : -INFINITY;
				m = fmaxf( m, v[ j ] );
			}
			const float inv = softMaxRowReg( v, m, shf, shd ).inv;
			RowStats st;
#pragma unroll
			for( int j = 0; j < SC_PER; j++ )
			{
				const int c = threadIdx.x + j * 1024;
				const float p = v[ j ] * inv;
				v[ j ] = p;
				if( c < nVocab )
				{
					if( probsOut ) probsOut[ (long long)blockIdx.x * nVocab + c ] = p;
					st.feed( p, c, tokenBeg, tsEnd );
				}
			}
			const bool onlyTs = st.reduce( forceTimestamp, sha, shd );
			const int lo = onlyTs ? tokenBeg : 0;
			ArgMax pick = { -INFINITY, 0 };
			for( int round = 0; round < 4; round++ )
			{
				ArgMax best = { -INFINITY, 0x7fffffff };
#pragma unroll
				for( int j = 0; j < SC_PER; j++ )
				{
					const int c = threadIdx.x + j * 1024;
					const bool ok = c < nVocab && c >= lo && !( c >= tsEnd && c >= tokenBeg );
					if( ok ) best = better( best, ArgMax{ v[ j ], c } );
				}
				best = blockArgMax<16>( best, sha );
				pick = best;
				// remove the winner from its owner's registers for the next round
#pragma unroll
				for( int j = 0; j < SC_PER; j++ )
					if( (int)threadIdx.x + j * 1024 == best.i ) v[ j ] = -INFINITY;
				if( !specialToken( best.i, tokenSot, tokenSolm, tokenNot ) ) break;
			}
			if( threadIdx.x == 0 ) publishSample( state, mail, out, nextTokens, sampleRecord( pick, st.ts, st.sumTs, nVocab ), blockIdx.x, gridDim.x );
		}

		// ---- the same sampler for the few rows of ONE stream, spread over the chip -------------------------------------
		// softMaxSampleKernel gives a row to one workgroup: 207 KB of logits and 52 k exponentials on ONE CU = 41 us of the ~1.1 ms a
		// single-stream token takes. Here a row is cut into SP_G slices: (1) slice maxima, (2) e = exp16( x - global max ), slice sums,
		// slice argmaxima and top-4 lists, (3) one wave per row merges the SP_G records and applies sampleBest's rules. Same values:
		// p = e * float( 1 / double sum ) for every number that leaves the sampler; the timestamp sum adds the same products in another order
		// (double). e (unnormalised) is left in `eOut`.
		constexpr int SP_G = 64;
		struct SamplePart
		{
			double sumE;
			ArgMax tx, ts;
			ArgMax topAll[ 4 ], topTs[ 4 ];
		};
		__global__ void __launch_bounds__( 256 ) sampleSpreadMax( const float* __restrict__ logits, int nVocab, float* __restrict__ partMax )
		{
			__shared__ float sh[ 4 ];
			const int row = blockIdx.y, g = blockIdx.x;
			const int per = ( nVocab + SP_G - 1 ) / SP_G;
			const int c0 = g * per, c1 = min( c0 + per, nVocab );
			const float* x = logits + (long long)row * nVocab;
			float m = -INFINITY;
			for( int c = c0 + threadIdx.x; c < c1; c += 256 ) m = fmaxf( m, x[ c ] );
			m = waveReduceMax( m );
			if( ( threadIdx.x & 63 ) == 0 ) sh[ threadIdx.x >> 6 ] = m;
			__syncthreads();
			if( threadIdx.x == 0 ) partMax[ row * SP_G + g ] = fmaxf( fmaxf( sh[ 0 ], sh[ 1 ] ), fmaxf( sh[ 2 ], sh[ 3 ] ) );
		}
		__global__ void __launch_bounds__( 256 ) sampleSpreadExp( const float* __restrict__ logits, int nVocab, int tokenBeg, const float* __restrict__ partMax,
			const DecodeState* __restrict__ state, float* __restrict__ eOut, SamplePart* __restrict__ parts )
		{
			__shared__ ArgMax sha[ 4 ];
			__shared__ double shd[ 4 ];
			const int row = blockIdx.y, g = blockIdx.x;
			const int per = ( nVocab + SP_G - 1 ) / SP_G;
			const int c0 = g * per, c1 = min( c0 + per, nVocab );
			const float* x = logits + (long long)row * nVocab;
			const int tsEnd = timestampEnd( state->isInitial, tokenBeg, nVocab );
			float m = partMax[ row * SP_G + ( threadIdx.x & ( SP_G - 1 ) ) ];
			m = waveReduceMax( m );
			constexpr int PER_T = 4;	   // ceil( 51866 / 64 / 256 )
			float v[ PER_T ];
			double s = 0.0;
			ArgMax tx = { -1.0f, 0x7fffffff }, ts = { -1.0f, 0x7fffffff };
#pragma unroll
			for( int j = 0; j < PER_T; j++ )
			{
				const int c = c0 + threadIdx.x + j * 256;
				float e = -1.0f;	   // below every real e: never wins an argmax
				if( c < c1 )
				{
					const float xv = x[ c ];
					e = ( xv == -INFINITY ) ? 0.0f : exp16( xv - m );
					eOut[ (long long)row * nVocab + c ] = e;
					s += (double)e;
					if( c < tokenBeg ) tx = better( tx, ArgMax{ e, c } );
					else if( c < tsEnd ) ts = better( ts, ArgMax{ e, c } );
				}
				v[ j ] = e;
			}
			s = waveReduceSumD( s );
			if( ( threadIdx.x & 63 ) == 0 ) shd[ threadIdx.x >> 6 ] = s;
			tx = blockArgMax<4>( tx, sha );	   // (its barriers also publish shd)
			ts = blockArgMax<4>( ts, sha );
			SamplePart p;
			p.sumE = ( shd[ 0 ] + shd[ 1 ] ) + ( shd[ 2 ] + shd[ 3 ] );
			p.tx = tx; p.ts = ts;
			// the slice's four best tokens among all that may be sampled, and among its timestamps: whichever list the row needs is merged later
			for( int list = 0; list < 2; list++ )
			{
				float w[ PER_T ];
#pragma unroll
				for( int j = 0; j < PER_T; j++ )
				{
					const int c = c0 + threadIdx.x + j * 256;
					const bool ok = c < c1 && !( c >= tsEnd && c >= tokenBeg ) && ( list == 0 || c >= tokenBeg );
					w[ j ] = ok ? v[ j ] : -2.0f;
				}
				for( int round = 0; round < 4; round++ )
				{
					ArgMax best = { -2.0f, 0x7fffffff };
#pragma unroll
					for( int j = 0; j < PER_T; j++ ) best = better( best, ArgMax{ w[ j ], c0 + (int)threadIdx.x + j * 256 } );
					best = blockArgMax<4>( best, sha );
					if( best.v < 0.0f ) best.i = 0x7fffffff;	   // the slice has fewer than `round + 1` such tokens
					( list == 0 ? p.topAll : p.topTs )[ round ] = best;
#pragma unroll
					for( int j = 0; j < PER_T; j++ )
						if( c0 + (int)threadIdx.x + j * 256 == best.i ) w[ j ] = -2.0f;
				}
			}
			if( threadIdx.x == 0 ) parts[ row * SP_G + g ] = p;
		}
		__global__ void __launch_bounds__( 64 ) sampleSpreadFinal( const SamplePart* __restrict__ parts, const float* __restrict__ e, int nVocab, int tokenBeg,
			int tokenSot, int tokenSolm, int tokenNot, const DecodeState* __restrict__ state, TokenData* __restrict__ out, int* __restrict__ nextTokens,
			const SampleMailbox mail )
		{
			static_assert( SP_G == 64, "one lane per slice" );
			const int row = blockIdx.x, lane = threadIdx.x;
			const SamplePart p = parts[ row * SP_G + lane ];
			const int forceTimestamp = state->forceTimestamp;
			const int tsEnd = timestampEnd( state->isInitial, tokenBeg, nVocab );
			const double sum = waveReduceSumD( p.sumE );
			const float inv = (float)( 1.0 / sum );
			ArgMax tx = waveArgMax( p.tx ), ts = waveArgMax( p.ts );
			tx.v = tx.v < 0.0f ? -1.0f : tx.v * inv;
			ts.v = ts.v < 0.0f ? -1.0f : ts.v * inv;
			// the timestamp probabilities once more, as the products the one-workgroup sampler adds
			double sumTs = 0.0;
			for( int c = tokenBeg + lane; c < tsEnd; c += 64 ) sumTs += (double)( e[ (long long)row * nVocab + c ] * inv );
			sumTs = waveReduceSumD( sumTs );
			const bool onlyTs = ( sumTs > (double)fmaxf( tx.v, -1.0f ) ) || forceTimestamp;
			// merge the slices' lists: every round the best head wins and its lane moves on
			ArgMax mine[ 4 ];
#pragma unroll
			for( int k = 0; k < 4; k++ ) mine[ k ] = onlyTs ? p.topTs[ k ] : p.topAll[ k ];
			int cursor = 0;
			ArgMax pick = { -INFINITY, 0 };
			for( int round = 0; round < 4; round++ )
			{
				ArgMax head = { -2.0f, 0x7fffffff };
#pragma unroll
				for( int k = 0; k < 4; k++ )
					if( k == cursor ) head = mine[ k ];
				if( head.i == 0x7fffffff ) head.v = -2.0f;
				const ArgMax best = waveArgMax( head );
				if( best.i == head.i && head.i != 0x7fffffff ) cursor++;
				pick = best;
				if( !specialToken( best.i, tokenSot, tokenSolm, tokenNot ) ) break;
			}
			if( lane == 0 )
			{
				if( pick.i < 0 || pick.i >= nVocab ) { pick.i = 0; pick.v = 0.0f; }
				pick.v = pick.v * inv;
				publishSample( state, mail, out, nextTokens, sampleRecord( pick, ts, sumTs, nVocab ), row, gridDim.x );
			}
		}

		// ---- no-speech probability of the prompt step (wh_decode_window_no_speech): out[ row ] = p[ tokenSolm ] of the row the sampler just left in `probs` ----
		// parts == nullptr: the row holds probabilities (softMaxSampleKernel, the scaled softmax). Otherwise it holds the spread sampler's unnormalised e, and
		// p = e * float( 1 / sum ) with the sum sampleSpreadFinal forms from the same slice records in the same order. One wave per row.
		__global__ void __launch_bounds__( 64 ) noSpeechGatherKernel( const float* __restrict__ probs, const SamplePart* __restrict__ parts, int nVocab, int tokenSolm,
			float* __restrict__ out )
		{
			static_assert( SP_G == 64, "one lane per slice" );
			const int row = blockIdx.x, lane = threadIdx.x;
			float v = probs[ (long long)row * nVocab + tokenSolm ];
			if( parts )
			{
				const double sum = waveReduceSumD( parts[ row * SP_G + lane ].sumE );
				v = v * (float)( 1.0 / sum );
			}
			if( lane == 0 ) out[ row ] = v;
		}

		__global__ void advanceStateKernel( DecodeState* state, int* seqPos, int rows )
		{
			const int i = blockIdx.x * blockDim.x + threadIdx.x;
			if( i < rows ) seqPos[ i ] += 1;
			if( i == 0 )
			{
				state->step += 1;
				state->forceTimestamp = 0;
				state->isInitial = 0;
			}
		}

		// ---- temperature sampling -----------------------------------------------------------------------------------
		// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), the counter-based generator of curand and torch:
		// the draw of a row depends on (seed, position, row, nonce) only -- not on the launch, the batch or what ran before
		struct Philox4 { unsigned x0, x1, x2, x3; };
		__device__ __forceinline__ Philox4 philox4x32_10( unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1 )
		{
			constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
			for( int r = 0; r < 10; r++ )
			{
				const unsigned hi0 = __umulhi( M0, c0 ), lo0 = M0 * c0;
				const unsigned hi1 = __umulhi( M1, c2 ), lo1 = M1 * c2;
				const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
				c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
				k0 += W0; k1 += W1;
			}
			return Philox4{ c0, c1, c2, c3 };
		}
		// 53 bits of the block -> [0, 1)
		__device__ __forceinline__ double philoxUniform( unsigned seedLo, unsigned seedHi, unsigned nonce, int position, int row )
		{
			const Philox4 x = philox4x32_10( (unsigned)position, (unsigned)row, nonce, 0u, seedLo, seedHi );
			const unsigned long long bits = ( (unsigned long long)x.x0 << 21 ) | (unsigned long long)( x.x1 >> 11 );
			return (double)bits * 0x1p-53;
		}

		__global__ void __launch_bounds__( 256 ) philoxUKernel( unsigned seedLo, unsigned seedHi, unsigned nonce, int rows, const int* __restrict__ positions,
			double* __restrict__ uOut )
		{
			const int row = blockIdx.x * 256 + threadIdx.x;
			if( row < rows ) uOut[ row ] = philoxUniform( seedLo, seedHi, nonce, positions[ row ], row );
		}

		struct DrawArgs
		{
			const float* probs;
			int nVocab, tokenBeg, tokenSot, tokenSolm, tokenNot;
			int forceTimestamp, isInitial;	   // state == nullptr: the flags of the call
			const DecodeState* state;		   // the greedy loop's device state: flags, output slot, mailbox generation
			unsigned seedLo, seedHi, nonce;	   // params == nullptr: the generator's key and nonce of the call
			const SampleParams* params;		   // device memory: a captured step graph outlives a change of seed or nonce
			const SampleRowParams* rowParams;  // device [rows] or nullptr: every row its own mode, key and nonce (wh_context_set_sampling_rows)
			const int* positions;			   // [rows]
			TokenData* out;					   // state ? [step][rows] : [rows]
			int* nextTokens;				   // [rows] or nullptr
			SampleMailbox mail;
		};

		// One 1024-thread workgroup per row, three passes over it (the row was just written by the softmax: it comes from L2):
		//   1. sampleBestKernel's own statistics in its own order (thread-strided sweep, blockArgMax, blockSumD): tx, ts, sumTs have its bits, so tid / pt / ptsum
		//      and the timestamp-vs-text decision are wh_op_sample_best's.
		//   2. the allowed mass in tiles of 64 consecutive columns: a wave owns a contiguous run of tiles, reads each coalesced and leaves its FP64 sum in LDS; a
		//      workgroup-wide scan over the <= 1024 tile sums (thread t = tile t) gives W and every tile's prefix, and the first tile whose prefix passes u W.
		//   3. wave 0 scans that one tile and takes the first column whose prefix passes u W.
		// Rounding may leave no column (u W rounds up to W, or the tile's scan falls an ulp short of its sum): then the last allowed column with p > 0 -- of the
		// tile, else of the row. W == 0 (or NaN): sampleBestKernel's pick. No atomics, no scratch; 8.4 KB of LDS.
		// With rowParams every row has its own record: a greedy row ends behind pass 1 with sampleBestKernel's pick (the branch is uniform over the workgroup, so
		// the barriers of passes 2 and 3 stay legal); a sampled row draws under its own key and nonce with the row word of the Philox counter 0 -- the draws of a
		// stream do not depend on the slot it sits in, and the row equals this kernel run on that row alone.
		__global__ void __launch_bounds__( 1024 ) sampleDrawKernel( const DrawArgs a )
		{
			__shared__ ArgMax sha[ 16 ];
			__shared__ double shd[ 16 ];
			__shared__ double tileSum[ 1024 ];
			__shared__ int shFirst[ 16 ], shLast[ 16 ];
			__shared__ double shExcl;
			__shared__ int shId;
			const int nVocab = a.nVocab, tokenBeg = a.tokenBeg, tokenSot = a.tokenSot, tokenSolm = a.tokenSolm, tokenNot = a.tokenNot;
			const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
			const float* const p = a.probs + (long long)row * nVocab;
			const int forceTimestamp = a.state ? a.state->forceTimestamp : a.forceTimestamp;
			const int isInitial = a.state ? a.state->isInitial : a.isInitial;
			const int tsEnd = timestampEnd( isInitial, tokenBeg, nVocab );

			// ---- 1: best text token and the timestamp statistics ----
			RowStats st;
			for( int c = tid; c < nVocab; c += 1024 ) st.feed( p[ c ], c, tokenBeg, tsEnd );
			const bool onlyTs = st.reduce( forceTimestamp, sha, shd );
			auto publish = [ & ]( ArgMax pick )
			{
				const TokenData r = sampleRecord( pick, st.ts, st.sumTs, nVocab );
				if( a.state ) publishSample( a.state, a.mail, a.out, a.nextTokens, r, row, gridDim.x );
				else
				{
					a.out[ row ] = r;
					if( a.nextTokens ) a.nextTokens[ row ] = r.id;
				}
			};
			SampleParams prm = { 1.0f, a.seedLo, a.seedHi, a.nonce };
			int philoxRow = row;
			if( a.rowParams )
			{
				const SampleRowParams rp = a.rowParams[ row ];
				if( !rp.sampled )
				{
					const ArgMax pick = sampleBestPick( p, nVocab, tokenBeg, tsEnd, onlyTs, tokenSot, tokenSolm, tokenNot, sha );
					if( tid == 0 ) publish( pick );
					return;
				}
				prm = SampleParams{ rp.invT, rp.seedLo, rp.seedHi, rp.nonce };
				philoxRow = 0;
			}
			else if( a.params ) prm = *a.params;
			auto allowed = [ & ]( int c ) -> bool
			{
				if( c >= tokenBeg ) return c < tsEnd;
				return !onlyTs && c != tokenSot && c != tokenSolm && c != tokenNot;
			};

			// ---- 2: tile sums, their scan, the tile the draw falls into ----
			const int nTiles = ( nVocab + 63 ) >> 6;
			const int perWave = ( nTiles + 15 ) >> 4;
			const int k1 = min( ( wave + 1 ) * perWave, nTiles );
			int lastPos = -1;
			for( int k = wave * perWave; k < k1; k++ )
			{
				const int c = k * 64 + lane;
				const bool ok = c < nVocab && allowed( c );
				const float v = ok ? p[ c ] : 0.0f;
				if( ok && v > 0.0f ) lastPos = c;
				const double s = waveReduceSumD( (double)v );
				if( lane == 0 ) tileSum[ k ] = s;
			}
			__syncthreads();
			const double mine = tid < nTiles ? tileSum[ tid ] : 0.0;
			double incl = mine;
#pragma unroll
			for( int o = 1; o < 64; o <<= 1 )
			{
				const double y = __shfl_up( incl, o, 64 );
				if( lane >= o ) incl += y;
			}
			double excl = __shfl_up( incl, 1, 64 );
			if( lane == 0 ) excl = 0.0;
			if( lane == 63 ) shd[ wave ] = incl;
#pragma unroll
			for( int o = 32; o > 0; o >>= 1 ) lastPos = max( lastPos, __shfl_xor( lastPos, o, 64 ) );
			if( lane == 0 ) shLast[ wave ] = lastPos;
			__syncthreads();
			double base = 0.0, W = 0.0;
			for( int i = 0; i < 16; i++ )
			{
				if( i == wave ) base = W;
				W += shd[ i ];
			}
			// tile t's prefix before it is exactly tile t - 1's prefix behind it: both are base + the wave's scan
			incl += base;
			excl += base;
			int rowLast = shLast[ 0 ];
			for( int i = 1; i < 16; i++ ) rowLast = max( rowLast, shLast[ i ] );

			const double u = philoxUniform( prm.seedLo, prm.seedHi, prm.nonce, a.positions[ row ], philoxRow );
			const double target = u * W;
			const bool hit = tid < nTiles && incl > target;
			const unsigned long long hits = __ballot( hit );
			if( lane == 0 ) shFirst[ wave ] = hits ? wave * 64 + __ffsll( (long long)hits ) - 1 : 0x7fffffff;
			__syncthreads();	  // (also: everyone has read shd)
			int tile = shFirst[ 0 ];
			for( int i = 1; i < 16; i++ ) tile = min( tile, shFirst[ i ] );
			if( tid == tile ) shExcl = excl;
			__syncthreads();

			ArgMax pick = { 0.0f, 0 };
			if( !( W > 0.0 ) )
			{
				// nothing to draw from: sampleBestKernel's pick
				pick = sampleBestPick( p, nVocab, tokenBeg, tsEnd, onlyTs, tokenSot, tokenSolm, tokenNot, sha );
			}
			else
			{
				// ---- 3: the column inside the tile ----
				if( wave == 0 )
				{
					int id = rowLast;
					if( tile != 0x7fffffff )
					{
						const int c = tile * 64 + lane;
						const bool ok = c < nVocab && allowed( c );
						const float v = ok ? p[ c ] : 0.0f;
						double cum = (double)v;
#pragma unroll
						for( int o = 1; o < 64; o <<= 1 )
						{
							const double y = __shfl_up( cum, o, 64 );
							if( lane >= o ) cum += y;
						}
						const unsigned long long pass = __ballot( ok && shExcl + cum > target );
						const unsigned long long positive = __ballot( ok && v > 0.0f );
						if( pass ) id = tile * 64 + __ffsll( (long long)pass ) - 1;
						else if( positive ) id = tile * 64 + 63 - __clzll( (long long)positive );
					}
					if( lane == 0 ) shId = id;
				}
				__syncthreads();
				pick.i = shId;
				if( pick.i < 0 || pick.i >= nVocab ) pick.i = 0;
				pick.v = p[ pick.i ];
			}

			if( tid == 0 ) publish( pick );
		}

		bool drawShapeOk( int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot )
		{
			return rows >= 1 && nVocab >= 1 && nVocab <= SAMPLE_DRAW_MAX_VOCAB && tokenBeg >= 1 && tokenBeg < nVocab && tokenSot >= 0 && tokenSot < tokenBeg &&
				tokenSolm >= 0 && tokenSolm < tokenBeg && tokenNot >= 0 && tokenNot < tokenBeg;
		}
	}	// namespace

	int launchSoftMaxRows( float* x, int rows, int cols, hipStream_t stream )
	{
		hipLaunchKernelGGL( softMaxRows<false>, dim3( rows ), dim3( 1024 ), 0, stream, x, x, cols, 1.0f, (const float*)nullptr );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchVocabSoftMax( const float* logits, float* probs, int rows, int nVocab, hipStream_t stream )
	{
		// option beam_regs: the row in registers (one read and one write instead of three reads and two writes), the same probabilities
		if( g_opt.beamRegs && nVocab <= SC_PER * 1024 )
			hipLaunchKernelGGL( softMaxRowsReg<false>, dim3( rows ), dim3( 1024 ), 0, stream, logits, probs, nVocab, 1.0f, (const float*)nullptr );
		else
			hipLaunchKernelGGL( softMaxRows<false>, dim3( rows ), dim3( 1024 ), 0, stream, logits, probs, nVocab, 1.0f, (const float*)nullptr );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchVocabSoftMaxScaled( const float* logits, float invT, const float* invTDev, float* probs, int rows, int nVocab, hipStream_t stream )
	{
		// the same choice of kernel as launchVocabSoftMax, so that the scaled row has the bits the unscaled kernels give on a host-scaled row
		if( g_opt.beamRegs && nVocab <= SC_PER * 1024 )
			hipLaunchKernelGGL( softMaxRowsReg<true>, dim3( rows ), dim3( 1024 ), 0, stream, logits, probs, nVocab, invT, invTDev );
		else
			hipLaunchKernelGGL( softMaxRows<true>, dim3( rows ), dim3( 1024 ), 0, stream, logits, probs, nVocab, invT, invTDev );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchNoSpeechGather( const float* probs, const void* spreadScratch, int rows, int nVocab, int tokenSolm, float* out, hipStream_t stream )
	{
		if( rows < 1 || tokenSolm < 0 || tokenSolm >= nVocab || !probs || !out ) { setError( "noSpeechGather: bad argument" ); return -1; }
		hipLaunchKernelGGL( noSpeechGatherKernel, dim3( rows ), dim3( 64 ), 0, stream, probs, (const SamplePart*)spreadScratch, nVocab, tokenSolm, out );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchLangProbs( const float* logits, long long rowStride, int rows, int nVocab, int tokenSot, int nLang, float* langP, int* best, hipStream_t stream )
	{
		if( rows < 1 || nLang < 1 || nLang > 1024 || tokenSot < 0 || (long long)tokenSot + 1 + nLang > nVocab || rowStride < nVocab || nVocab > SC_PER * 1024 )
		{
			setError( "langProbs: the language block must lie inside the row and hold 1 .. 1024 tokens, the vocabulary at most 52224" );
			return -1;
		}
		hipLaunchKernelGGL( langProbsKernel, dim3( rows ), dim3( 1024 ), 0, stream, logits, rowStride, nVocab, tokenSot, nLang, langP, best );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchTokenScores( const float* logits, long long rowStride, int rows, int nVocab, const int* targets, TokenScore* out, hipStream_t stream )
	{
		if( !logits || !targets || !out || rows < 1 || nVocab < 1 || rowStride < nVocab ) { setError( "tokenScores: bad argument" ); return -1; }
		// option score_regs: the row in registers where it fits (one read), two reads beyond and with the option off; the same bits
		if( g_opt.scoreRegs && nVocab <= SC_PER * 1024 )
			hipLaunchKernelGGL( tokenScoreKernel<true>, dim3( rows ), dim3( 1024 ), 0, stream, logits, rowStride, nVocab, targets, out );
		else
			hipLaunchKernelGGL( tokenScoreKernel<false>, dim3( rows ), dim3( 1024 ), 0, stream, logits, rowStride, nVocab, targets, out );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchGatherScoreRows( const f16* x, const int* tokens, const int* meta, int windows, int nMax, int d, f16* dst, int* targets, hipStream_t stream )
	{
		if( !x || !tokens || !meta || !dst || !targets || windows < 1 || windows > 65535 || nMax < 2 || d < 8 || ( d % 8 ) != 0 ) { setError( "gatherScoreRows: bad argument" ); return -1; }
		hipLaunchKernelGGL( gatherScoreRowsKernel, dim3( nMax - 1, windows ), dim3( 128 ), 0, stream, x, tokens, meta, windows, nMax, d, dst, targets );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchLangGather( const float* probs, long long rowStride, int rows, int nVocab, int tokenSot, int nLang, float* langP, int* best, hipStream_t stream )
	{
		if( rows < 1 || nLang < 1 || nLang > 1024 || tokenSot < 0 || (long long)tokenSot + 1 + nLang > nVocab || rowStride < nVocab )
		{
			setError( "langGather: the language block must lie inside the row and hold 1 .. 1024 tokens" );
			return -1;
		}
		hipLaunchKernelGGL( langGatherKernel, dim3( rows ), dim3( 1024 ), 0, stream, probs, rowStride, tokenSot, nLang, langP, best );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchSampleBest( const float* probs, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot,
		int forceTimestamp, int isInitial, TokenData* out, hipStream_t stream )
	{
		hipLaunchKernelGGL( sampleBestKernel, dim3( rows ), dim3( 1024 ), 0, stream, probs, nVocab, tokenBeg, tokenSot, tokenSolm,
			tokenNot, forceTimestamp, isInitial, out );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchBeamCandidates( const float* probs, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot,
		int forceTimestamp, int isInitial, int width, TokenData* out, hipStream_t stream )
	{
		if( width < 1 || width > 8 ) { setError( "beamCandidates: width must be 1 .. 8" ); return -1; }
		hipLaunchKernelGGL( beamCandidatesKernel, dim3( rows ), dim3( 1024 ), 0, stream, probs, nVocab, tokenBeg, tokenSot, tokenSolm,
			tokenNot, forceTimestamp, isInitial, width, out );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchSoftMaxSample( const float* logits, float* probsOut, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm,
		int tokenNot, const DecodeState* state, TokenData* out, int* nextTokens, SampleMailbox mail, hipStream_t stream )
	{
		if( nVocab > SC_PER * 1024 )
		{
			setError( "softMaxSample: vocabulary larger than 52224" );
			return -1;
		}
		hipLaunchKernelGGL( softMaxSampleKernel, dim3( rows ), dim3( 1024 ), 0, stream, logits, probsOut, nVocab, tokenBeg, tokenSot, tokenSolm,
			tokenNot, state, out, nextTokens, mail );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	size_t sampleSpreadScratchBytes( int rows ) { return (size_t)rows * SP_G * ( sizeof( SamplePart ) + sizeof( float ) ); }
	int launchSoftMaxSampleSpread( const float* logits, float* eOut, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot,
		const DecodeState* state, TokenData* out, int* nextTokens, SampleMailbox mail, void* scratch, hipStream_t stream )
	{
		if( nVocab > SP_G * 256 * 4 || rows < 1 || !scratch || !eOut ) { setError( "softMaxSampleSpread: bad argument" ); return -1; }
		SamplePart* const parts = (SamplePart*)scratch;
		float* const partMax = (float*)( parts + (size_t)rows * SP_G );
		hipLaunchKernelGGL( sampleSpreadMax, dim3( SP_G, rows ), dim3( 256 ), 0, stream, logits, nVocab, partMax );
		hipLaunchKernelGGL( sampleSpreadExp, dim3( SP_G, rows ), dim3( 256 ), 0, stream, logits, nVocab, tokenBeg, partMax, state, eOut, parts );
		hipLaunchKernelGGL( sampleSpreadFinal, dim3( rows ), dim3( 64 ), 0, stream, parts, eOut, nVocab, tokenBeg, tokenSot, tokenSolm, tokenNot, state, out,
			nextTokens, mail );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchAdvanceState( DecodeState* state, int* seqPos, int rows, hipStream_t stream )
	{
		hipLaunchKernelGGL( advanceStateKernel, dim3( ( rows + 127 ) / 128 ), dim3( 128 ), 0, stream, state, seqPos, rows );
		WH_HIP( hipGetLastError() );
		return 0;
	}
	int launchSampleDraw( const float* probs, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot, int forceTimestamp, int isInitial,
		unsigned long long seed, unsigned nonce, const int* positions, TokenData* out, hipStream_t stream )
	{
		if( !probs || !positions || !out || !drawShapeOk( rows, nVocab, tokenBeg, tokenSot, tokenSolm, tokenNot ) )
		{
			setError( "sampleDraw: bad pointer, token id or size (at most 65536 columns)" );
			return -1;
		}
		DrawArgs a = {};
		a.probs = probs; a.nVocab = nVocab; a.tokenBeg = tokenBeg; a.tokenSot = tokenSot; a.tokenSolm = tokenSolm; a.tokenNot = tokenNot;
		a.forceTimestamp = forceTimestamp; a.isInitial = isInitial;
		a.seedLo = (unsigned)( seed & 0xffffffffull ); a.seedHi = (unsigned)( seed >> 32 ); a.nonce = nonce;
		a.positions = positions; a.out = out;
		hipLaunchKernelGGL( sampleDrawKernel, dim3( rows ), dim3( 1024 ), 0, stream, a );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchSampleDrawStep( const float* probs, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot, const DecodeState* state,
		const SampleParams* params, const int* positions, TokenData* out, int* nextTokens, SampleMailbox mail, hipStream_t stream )
	{
		if( !probs || !positions || !out || !state || !params || !nextTokens || !drawShapeOk( rows, nVocab, tokenBeg, tokenSot, tokenSolm, tokenNot ) )
		{
			setError( "sampleDrawStep: bad pointer, token id or size (at most 65536 columns)" );
			return -1;
		}
		DrawArgs a = {};
		a.probs = probs; a.nVocab = nVocab; a.tokenBeg = tokenBeg; a.tokenSot = tokenSot; a.tokenSolm = tokenSolm; a.tokenNot = tokenNot;
		a.state = state; a.params = params; a.positions = positions; a.out = out; a.nextTokens = nextTokens; a.mail = mail;
		hipLaunchKernelGGL( sampleDrawKernel, dim3( rows ), dim3( 1024 ), 0, stream, a );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchVocabSoftMaxRows( const float* logits, const SampleRowParams* rowParams, float* probs, int rows, int nVocab, hipStream_t stream )
	{
		if( !logits || !rowParams || !probs || rows < 1 || nVocab < 1 ) { setError( "vocabSoftMaxRows: bad argument" ); return -1; }
		// the same choice of kernel as launchVocabSoftMax, so that a greedy row (factor 1) has its bits
		if( g_opt.beamRegs && nVocab <= SC_PER * 1024 )
			hipLaunchKernelGGL( ( softMaxRowsReg<true, true> ), dim3( rows ), dim3( 1024 ), 0, stream, logits, probs, nVocab, 1.0f, &rowParams->invT );
		else
			hipLaunchKernelGGL( ( softMaxRows<true, true> ), dim3( rows ), dim3( 1024 ), 0, stream, logits, probs, nVocab, 1.0f, &rowParams->invT );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchSampleRows( const float* probs, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot, int forceTimestamp, int isInitial,
		const DecodeState* state, const SampleRowParams* rowParams, const int* positions, TokenData* out, int* nextTokens, SampleMailbox mail, hipStream_t stream )
	{
		if( !probs || !positions || !out || !rowParams || ( state && !nextTokens ) || !drawShapeOk( rows, nVocab, tokenBeg, tokenSot, tokenSolm, tokenNot ) )
		{
			setError( "sampleRows: bad pointer, token id or size (at most 65536 columns)" );
			return -1;
		}
		DrawArgs a = {};
		a.probs = probs; a.nVocab = nVocab; a.tokenBeg = tokenBeg; a.tokenSot = tokenSot; a.tokenSolm = tokenSolm; a.tokenNot = tokenNot;
		a.forceTimestamp = forceTimestamp; a.isInitial = isInitial;
		a.state = state; a.rowParams = rowParams; a.positions = positions; a.out = out; a.nextTokens = nextTokens; a.mail = mail;
		hipLaunchKernelGGL( sampleDrawKernel, dim3( rows ), dim3( 1024 ), 0, stream, a );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchPhiloxU( unsigned long long seed, unsigned nonce, int rows, const int* positions, double* uOut, hipStream_t stream )
	{
		if( rows < 1 || !positions || !uOut ) { setError( "philoxU: bad argument" ); return -1; }
		hipLaunchKernelGGL( philoxUKernel, dim3( ( rows + 255 ) / 256 ), dim3( 256 ), 0, stream, (unsigned)( seed & 0xffffffffull ), (unsigned)( seed >> 32 ), nonce, rows,
			positions, uOut );
		WH_HIP( hipGetLastError() );
		return 0;
	}
}
