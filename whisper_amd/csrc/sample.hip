// Temperature sampling: one categorical draw per row of probabilities under ContextImpl::sampleBest's own masks ("Decoding fallback").
// The reference has no temperature anywhere; the rules are this project's and are restated in float64 by tests/fallback_ref.py.
#include "kernels.h"
#include "block_reduce.h"

namespace wh
{
	namespace
	{
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
			const int tsEnd = isInitial ? min( tokenBeg + 101, nVocab ) : nVocab;

			// ---- 1: best text token and the timestamp statistics, exactly as sampleBestKernel forms them ----
			ArgMax tx = { -1.0f, 0x7fffffff }, ts = { -1.0f, 0x7fffffff };
			double sumTs = 0.0;
			for( int c = tid; c < nVocab; c += 1024 )
			{
				const float v = p[ c ];
				if( c < tokenBeg )
					tx = better( tx, ArgMax{ v, c } );
				else if( c < tsEnd )
				{
					ts = better( ts, ArgMax{ v, c } );
					sumTs += (double)v;
				}
			}
			tx = blockArgMax( tx, sha );
			ts = blockArgMax( ts, sha );
			sumTs = blockSumD<16>( sumTs, shd );
			const bool onlyTs = ( sumTs > (double)fmaxf( tx.v, -1.0f ) ) || forceTimestamp;
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

			const SampleParams prm = a.params ? *a.params : SampleParams{ 1.0f, a.seedLo, a.seedHi, a.nonce };
			const double u = philoxUniform( prm.seedLo, prm.seedHi, prm.nonce, a.positions[ row ], row );
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
				// nothing to draw from: sampleBestKernel's pick -- the top 4 under the mask, the first that is not sot / solm / not
				const int lo = onlyTs ? tokenBeg : 0;
				int taken[ 4 ];
				for( int round = 0; round < 4; round++ )
				{
					ArgMax best = { -INFINITY, 0x7fffffff };
					for( int c = lo + tid; c < nVocab; c += 1024 )
					{
						bool skip = c >= tsEnd && c >= tokenBeg;
						for( int k = 0; k < round; k++ ) skip = skip || ( taken[ k ] == c );
						if( !skip ) best = better( best, ArgMax{ p[ c ], c } );
					}
					best = blockArgMax( best, sha );
					taken[ round ] = best.i;
					pick = best;
					const bool special = best.i == tokenSot || best.i == tokenSolm || best.i == tokenNot;
					if( !special ) break;
				}
				if( pick.i < 0 || pick.i >= nVocab ) pick.i = 0;
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

			if( tid == 0 )
			{
				TokenData r;
				r.id = pick.i;
				r.tid = ts.v > -1.0f ? ts.i : 0;
				r.p = pick.v;
				r.pt = (float)( (double)ts.v / ( sumTs + 1e-10 ) );
				r.ptsum = (float)sumTs;
				if( !a.state )
				{
					a.out[ row ] = r;
					if( a.nextTokens ) a.nextTokens[ row ] = r.id;
					return;
				}
				// the greedy loop's bookkeeping, as softMaxSampleKernel does it: the sample's slot, the token the next step embeds, the host mailbox
				const long long slot = (long long)a.state->step * gridDim.x + row;
				a.out[ slot ] = r;
				a.nextTokens[ row ] = r.id;
				const int gen = a.state->gen;
				if( a.mail.data && gen != 0 )
				{
					// the record as write-through stores, drained, then the stamp the host polls; the checksum lets a host that saw the stamp early reject a torn record
					int* const md = (int*)( a.mail.data + slot );
					__hip_atomic_store( md + 0, r.id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
					__hip_atomic_store( md + 1, r.tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
					__hip_atomic_store( md + 2, __float_as_int( r.p ), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
					__hip_atomic_store( md + 3, __float_as_int( r.pt ), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
					__hip_atomic_store( md + 4, __float_as_int( r.ptsum ), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
					const int check = (int)( (unsigned)gen ^ (unsigned)r.id ^ ( (unsigned)r.tid * 0x9E3779B1u ) ^ (unsigned)__float_as_int( r.p ) ^
						( (unsigned)__float_as_int( r.pt ) * 3u ) ^ ( (unsigned)__float_as_int( r.ptsum ) * 5u ) );
					__hip_atomic_store( a.mail.flag + 2 * slot + 1, check, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
					asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
					__hip_atomic_store( a.mail.flag + 2 * slot, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
				}
			}
		}

		bool drawShapeOk( int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot )
		{
			return rows >= 1 && nVocab >= 1 && nVocab <= SAMPLE_DRAW_MAX_VOCAB && tokenBeg >= 1 && tokenBeg < nVocab && tokenSot >= 0 && tokenSot < tokenBeg &&
				tokenSolm >= 0 && tokenSolm < tokenBeg && tokenNot >= 0 && tokenNot < tokenBeg;
		}
	}	// namespace

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

	int launchPhiloxU( unsigned long long seed, unsigned nonce, int rows, const int* positions, double* uOut, hipStream_t stream )
	{
		if( rows < 1 || !positions || !uOut ) { setError( "philoxU: bad argument" ); return -1; }
		hipLaunchKernelGGL( philoxUKernel, dim3( ( rows + 255 ) / 256 ), dim3( 256 ), 0, stream, (unsigned)( seed & 0xffffffffull ), (unsigned)( seed >> 32 ), nonce, rows,
			positions, uOut );
		WH_HIP( hipGetLastError() );
		return 0;
	}
}
