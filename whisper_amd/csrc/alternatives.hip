// Token alternatives (wh_context_set_alternatives; DESIGN.md section 7 "Token alternatives"): the k likeliest tokens of every row the sampler of the device-side
// loop sees, with their log-probabilities, as a by-product of the step. The kernel, its launch, the op-level entry and the owner of the context's ring.
#include "runtime.h"

namespace wh
{
	namespace
	{
		// ---- the k largest logits of a row and their log-probabilities (restated in float64 by tests/alternatives_ref.py) ----
		// Per row: lse = max + log( sum exp( x - max ) ) -- FP32 expf per term, the sum in double: thread by thread over its own elements in ascending id, the 64 lanes
		// of a wave by waveReduceSumD, the 16 waves one after the other -- and k records { id, float( double( x ) - lse ) }, the largest logits first, equal values in
		// ascending id. -inf and NaN are never listed (a NaN is read as -inf, in the sum too); when fewer than k entries are finite the rest is { -1, -inf }.
		// One 1024-thread workgroup per row and ONE read of the row: it stays in registers, 13 float4 per thread plus one scalar. Rows start at 4-byte alignment
		// (nVocab = 51865: every odd row), so the row is peeled: `head` = 0 .. 3 floats up to the first 16-byte boundary (threads 0 .. 2, scalar loads), nVec float4 from
		// there (thread t owns vectors t, t + 1024, ...: a wave reads 1 KB per load, all 13 loads issued before the first use), and 0 .. 3 floats behind them
		// (threads 4 .. 6). nVocab <= ALT_MAX_VOCAB = 13 * 4 * 1024, which bounds nVec whatever the alignment.
		// Selection: every thread keeps the best of its elements as ONE 64-bit key, ( ordered value bits << 32 ) | ~id: the larger key is the larger value and, among
		// equal values, the lower id, so a tie costs nothing. A round is the workgroup's maximum key -- 6 shuffles in the wave, one LDS slot per wave, one barrier (the
		// slots are double-buffered), 4 more shuffles -- and then only the thread that owned the winner clears that element and scans its 53 values again: one wave
		// diverges for ~110 instructions, the other 15 go straight to the next round. Key 0 is "nothing left". The first round's winner is the row maximum, which
		// the sum needs; k is the number of rounds and nothing before or between them depends on it, nor on the other rows: the first j records are the same bits
		// for every k >= j, alone or in a batch.
		// The records leave by thread 0 as 8-byte vector stores. state non-null (a step of the device-side loop): the records of row r go to
		// out[ ( state->step * rows + r ) * k ], the slot the sampler gives the row's wh_token_data; a step index outside [0, maxSteps) writes nothing.
		// Built, measured and NOT chosen: per-thread sorted insertion (topLogprobsInsertKernel below: 8 keys per thread while the row streams past, the same rounds
		// over the lists' heads; 56 VGPRs) -- 41.7 / 45.9 / 49.1 us at 1 row and 78.2 / 83.7 / 87.5 us at 448 x 51865 for k = 1 / 5 / 8, against 13.4 / 21.3 / 27.0
		// and 35.6 / 50.6 / 62.7 us for this kernel: with 64 lanes in step nearly every element costs the wave the whole insertion, VALU-bound.
		// Resource usage on gfx950 (kernel-resource-usage remark): 95 VGPRs, no scratch, 384 bytes of LDS. Measured: profiles/alternatives_probe.json.
		constexpr int ALT_THREADS = 1024, ALT_VEC = 13;
		static_assert( ALT_VEC * 4 * ALT_THREADS == ALT_MAX_VOCAB, "the row in registers" );
		using u64 = unsigned long long;

		__device__ __forceinline__ float altClean( float x ) { return x > -INFINITY ? x : -INFINITY; }	  // NaN compares false
		__device__ __forceinline__ u64 altKey( float v, int id )
		{
			if( !( v > -INFINITY ) ) return 0ull;
			const unsigned b = __float_as_uint( v );
			const unsigned ord = ( b & 0x80000000u ) ? ~b : ( b | 0x80000000u );
			return ( (u64)ord << 32 ) | (u64)(unsigned)~id;
		}
		__device__ __forceinline__ float altKeyValue( u64 key )
		{
			const unsigned ord = (unsigned)( key >> 32 );
			return __uint_as_float( ( ord & 0x80000000u ) ? ( ord ^ 0x80000000u ) : ~ord );
		}
		__device__ __forceinline__ u64 altMax( u64 a, u64 b ) { return a > b ? a : b; }
		// the maximum of the workgroup's keys in every lane; sh holds 16 slots that nobody writes again before the next barrier but one
		__device__ __forceinline__ u64 altBlockMax( u64 key, u64* sh )
		{
#pragma unroll
			for( int o = 32; o > 0; o >>= 1 ) key = altMax( key, __shfl_xor( key, o, 64 ) );
			if( ( threadIdx.x & 63 ) == 0 ) sh[ threadIdx.x >> 6 ] = key;
			__syncthreads();
			key = sh[ threadIdx.x & 15 ];
#pragma unroll
			for( int o = 8; o > 0; o >>= 1 ) key = altMax( key, __shfl_xor( key, o, 64 ) );
			return key;
		}
		// the best of a thread's elements: the vectors in ascending id with a strict compare, then the scalar under the key's own order
		__device__ __forceinline__ u64 altLocalBest( const float4 ( &v )[ ALT_VEC ], float extra, int extraId, int id0 )
		{
			float best = -INFINITY;
			int at = 0;
#pragma unroll
			for( int i = 0; i < ALT_VEC; i++ )
			{
				if( v[ i ].x > best ) { best = v[ i ].x; at = 4 * i; }
				if( v[ i ].y > best ) { best = v[ i ].y; at = 4 * i + 1; }
				if( v[ i ].z > best ) { best = v[ i ].z; at = 4 * i + 2; }
				if( v[ i ].w > best ) { best = v[ i ].w; at = 4 * i + 3; }
			}
			// slot 4 * i + j of thread t is element id0 + 4096 * i + j
			return altMax( altKey( best, id0 + ( at >> 2 ) * ( 4 * ALT_THREADS ) + ( at & 3 ) ), altKey( extra, extraId ) );
		}

		__global__ void __launch_bounds__( ALT_THREADS ) topLogprobsKernel( const float* __restrict__ logits, long long rowStride, int nVocab, int k,
			const DecodeState* __restrict__ state, int maxSteps, TokenAlternative* __restrict__ out )
		{
			__shared__ u64 shk[ 2 ][ 16 ];
			__shared__ double shd[ 16 ];
			const int t = threadIdx.x, row = blockIdx.x;
			const float* const x = logits + (long long)row * rowStride;
			const int head = min( (int)( ( 4u - ( (unsigned)( (size_t)x >> 2 ) & 3u ) ) & 3u ), nVocab );
			const int nVec = ( nVocab - head ) >> 2;
			const int tail0 = head + 4 * nVec;		  // the first element behind the vectors
			const float4* const xv = (const float4*)( x + head );
			float4 v[ ALT_VEC ];
#pragma unroll
			for( int i = 0; i < ALT_VEC; i++ )
			{
				const int j = t + ALT_THREADS * i;
				v[ i ] = make_float4( -INFINITY, -INFINITY, -INFINITY, -INFINITY );
				if( j < nVec ) v[ i ] = xv[ j ];
			}
			int extraId = -1;
			if( t < head ) extraId = t;
			else if( t >= 4 && tail0 + ( t - 4 ) < nVocab ) extraId = tail0 + ( t - 4 );
			float extra = -INFINITY;
			if( extraId >= 0 ) extra = altClean( x[ extraId ] );
#pragma unroll
			for( int i = 0; i < ALT_VEC; i++ ) v[ i ] = make_float4( altClean( v[ i ].x ), altClean( v[ i ].y ), altClean( v[ i ].z ), altClean( v[ i ].w ) );
			const int id0 = head + 4 * t;

			u64 mine = altLocalBest( v, extra, extraId, id0 );
			u64 win = altBlockMax( mine, shk[ 0 ] );
			// the row maximum is the first winner's value; a row without a finite entry has no sum
			const float m = win ? altKeyValue( win ) : 0.0f;
			double s = 0.0;
			if( t < head ) s += (double)expf( extra - m );
#pragma unroll
			for( int i = 0; i < ALT_VEC; i++ )
			{
				s += (double)expf( v[ i ].x - m );
				s += (double)expf( v[ i ].y - m );
				s += (double)expf( v[ i ].z - m );
				s += (double)expf( v[ i ].w - m );
			}
			if( t >= 4 ) s += (double)expf( extra - m );
			s = waveReduceSumD( s );
			if( ( t & 63 ) == 0 ) shd[ t >> 6 ] = s;
			__syncthreads();
			double lse = 0.0;
			long long slot = row;
			bool store = t == 0;
			if( t == 0 )
			{
				double sum = shd[ 0 ];
				for( int i = 1; i < 16; i++ ) sum += shd[ i ];
				lse = (double)m + log( sum );
				if( state )
				{
					const int step = state->step;
					store = step >= 0 && step < maxSteps;
					slot = (long long)step * gridDim.x + row;
				}
			}
			TokenAlternative* const o = out + slot * k;
			for( int r = 0; r < k; r++ )
			{
				if( r > 0 ) win = altBlockMax( mine, shk[ r & 1 ] );
				if( store )
				{
					TokenAlternative rec = { -1, -INFINITY };
					if( win )
					{
						rec.id = (int)~(unsigned)win;
						rec.logprob = (float)( (double)altKeyValue( win ) - lse );
					}
					o[ r ] = rec;
				}
				if( win != 0 && win == mine && r + 1 < k )
				{
					// keys are unique: this thread owns the winner. Out of its registers, then its next best
					const int id = (int)~(unsigned)win;
					if( id == extraId ) extra = -INFINITY;
					else
					{
						const int rel = id - id0, vi = rel / ( 4 * ALT_THREADS ), vj = rel & 3;
#pragma unroll
						for( int i = 0; i < ALT_VEC; i++ )
							if( i == vi )
							{
								if( vj == 0 ) v[ i ].x = -INFINITY;
								if( vj == 1 ) v[ i ].y = -INFINITY;
								if( vj == 2 ) v[ i ].z = -INFINITY;
								if( vj == 3 ) v[ i ].w = -INFINITY;
							}
					}
					mine = altLocalBest( v, extra, extraId, id0 );
				}
			}
		}

		// ---- the other form, kept for the measurement only (wh_debug_probe kind 5 variant 10; no caller besides it) ----
		// Per-thread sorted insertion: the row streams past, nothing of it stays in registers. Every thread keeps its 8 best keys sorted (one compare against the
		// smallest per element, then up to 7 compare-and-swaps) and a running maximum with the double sum rescaled to it (an online softmax: the same lse up to
		// rounding, not the same bits). The merge is the rounds above over the lists' heads; the winner's owner shifts its list. Any nVocab.
		struct AltList
		{
			u64 top[ ALT_MAX_K ];
			float m;
			double s;
			__device__ __forceinline__ void feed( float x, int id )
			{
				const float v = altClean( x );
				if( v > m ) { s = s * (double)expf( m - v ) + 1.0; m = v; }
				else if( v > -INFINITY ) s += (double)expf( v - m );
				const u64 key = altKey( v, id );
				if( key > top[ ALT_MAX_K - 1 ] )
				{
					top[ ALT_MAX_K - 1 ] = key;
#pragma unroll
					for( int i = ALT_MAX_K - 1; i > 0; i-- )
						if( top[ i ] > top[ i - 1 ] ) { const u64 t = top[ i ]; top[ i ] = top[ i - 1 ]; top[ i - 1 ] = t; }
				}
			}
		};
		__global__ void __launch_bounds__( ALT_THREADS ) topLogprobsInsertKernel( const float* __restrict__ logits, long long rowStride, int nVocab, int k,
			TokenAlternative* __restrict__ out )
		{
			__shared__ u64 shk[ 2 ][ 16 ];
			__shared__ double shd[ 16 ];
			const int t = threadIdx.x, row = blockIdx.x;
			const float* const x = logits + (long long)row * rowStride;
			const int head = min( (int)( ( 4u - ( (unsigned)( (size_t)x >> 2 ) & 3u ) ) & 3u ), nVocab );
			const int nVec = ( nVocab - head ) >> 2, tail0 = head + 4 * nVec;
			const float4* const xv = (const float4*)( x + head );
			AltList a;
#pragma unroll
			for( int i = 0; i < ALT_MAX_K; i++ ) a.top[ i ] = 0ull;
			a.m = -INFINITY;
			a.s = 0.0;
			if( t < head ) a.feed( x[ t ], t );
			for( int j = t; j < nVec; j += ALT_THREADS )
			{
				const float4 v = xv[ j ];
				const int id = head + 4 * j;
				a.feed( v.x, id ); a.feed( v.y, id + 1 ); a.feed( v.z, id + 2 ); a.feed( v.w, id + 3 );
			}
			if( t >= 4 && tail0 + ( t - 4 ) < nVocab ) a.feed( x[ tail0 + ( t - 4 ) ], tail0 + ( t - 4 ) );
			u64 win = altBlockMax( a.top[ 0 ], shk[ 0 ] );
			const float m = win ? altKeyValue( win ) : 0.0f;
			double s = a.m > -INFINITY ? a.s * (double)expf( a.m - m ) : 0.0;
			s = waveReduceSumD( s );
			if( ( t & 63 ) == 0 ) shd[ t >> 6 ] = s;
			__syncthreads();
			double lse = 0.0;
			if( t == 0 )
			{
				double sum = shd[ 0 ];
				for( int i = 1; i < 16; i++ ) sum += shd[ i ];
				lse = (double)m + log( sum );
			}
			TokenAlternative* const o = out + (long long)row * k;
			for( int r = 0; r < k; r++ )
			{
				if( r > 0 ) win = altBlockMax( a.top[ 0 ], shk[ r & 1 ] );
				if( t == 0 )
				{
					TokenAlternative rec = { -1, -INFINITY };
					if( win )
					{
						rec.id = (int)~(unsigned)win;
						rec.logprob = (float)( (double)altKeyValue( win ) - lse );
					}
					o[ r ] = rec;
				}
				if( win != 0 && win == a.top[ 0 ] )
				{
#pragma unroll
					for( int i = 0; i + 1 < ALT_MAX_K; i++ ) a.top[ i ] = a.top[ i + 1 ];
					a.top[ ALT_MAX_K - 1 ] = 0ull;
				}
			}
		}
	}	// namespace

	int launchTopLogprobsInsert( const float* logits, long long rowStride, int rows, int nVocab, int k, TokenAlternative* out, hipStream_t stream )
	{
		if( !logits || !out || rows < 1 || nVocab < 1 || rowStride < nVocab || k < 1 || k > ALT_MAX_K ) { setError( "topLogprobsInsert: bad argument" ); return -1; }
		hipLaunchKernelGGL( topLogprobsInsertKernel, dim3( rows ), dim3( ALT_THREADS ), 0, stream, logits, rowStride, nVocab, k, out );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchTopLogprobs( const float* logits, long long rowStride, int rows, int nVocab, int k, const DecodeState* state, int maxSteps, TokenAlternative* out, hipStream_t stream )
	{
		if( !logits || !out || rows < 1 || nVocab < 1 || nVocab > ALT_MAX_VOCAB || rowStride < nVocab || k < 1 || k > ALT_MAX_K || ( state && maxSteps < 1 ) )
		{
			setError( "topLogprobs: bad argument" );
			return -1;
		}
		hipLaunchKernelGGL( topLogprobsKernel, dim3( rows ), dim3( ALT_THREADS ), 0, stream, logits, rowStride, nVocab, k, state, maxSteps, out );
		WH_HIP( hipGetLastError() );
		return 0;
	}
}	// namespace wh

static int refuse( const std::string& text ) { setError( text.c_str() ); return WH_E_INVALIDARG; }

// ---- the owner of wh_context::altK, altRing and windowAltK ----------------------------------------------------
// One launch per step of the device-side loop, behind the sampler and in front of the advance: the row is the one the filters left and the sampler read, the step
// index is still the sample's, and the sampler's mailbox stamp has left before it. Accounted under the sampler's class.
int wh::alternativesStep( wh_context* c, int batch, bool windowStart )
{
	if( windowStart ) c->windowAltK = c->altK;	  // what wh_decode_window_alternatives holds the read against
	if( !c->altK ) return 0;
	const wh_hparams& hp = c->m->hp;
	return profiled( c, KC_SAMPLE, 20.0 * batch * hp.n_vocab, 4.0 * batch * hp.n_vocab,
		[ & ]() { return launchTopLogprobs( c->logits, hp.n_vocab, batch, hp.n_vocab, c->altK, c->state, hp.n_text_ctx, c->altRing, c->stream ); } );
}
// stepKey's bits of a step of the greedy loop: k in bits 22-25, which only a beam step's width uses otherwise. k is the kernel's argument and the ring's stride, so
// no graph serves another k; step_graph.hip keeps the graphs of k = 0 next to those of one k above it.
uint32_t wh::alternativesLoopKey( const wh_context* c ) { return (uint32_t)c->altK << 22; }
int wh::alternativesAllowFlags( const wh_context* c, uint32_t flags )
{
	return ( flags & WH_FLAG_PARITY_EXACT ) && c->altK ? refuse( "context_set_flags: WH_FLAG_PARITY_EXACT is not available while wh_context_set_alternatives is on" ) : 0;
}

extern "C" {

int wh_op_top_logprobs( void* stream, const float* logitsDev, int64_t rowStride, int rows, int nVocab, int k, wh_token_alternative* outDev )
{
	static_assert( sizeof( wh_token_alternative ) == sizeof( TokenAlternative ) && sizeof( wh_token_alternative ) == 8, "token alternative layout" );
	if( !logitsDev || !outDev ) return refuse( "top_logprobs: null logits or null output" );
	if( k < 1 || k > ALT_MAX_K ) return refuse( "top_logprobs: k outside 1 .. 8" );
	if( rows < 1 || nVocab < 1 ) return refuse( "top_logprobs: rows < 1 or nVocab < 1" );
	if( nVocab > ALT_MAX_VOCAB ) return refuse( "top_logprobs: more than 53248 columns (the row is held in registers)" );
	if( rowStride < nVocab ) return refuse( "top_logprobs: rowStride < nVocab" );
	return launchTopLogprobs( logitsDev, rowStride, rows, nVocab, k, nullptr, 0, (TokenAlternative*)outDev, (hipStream_t)stream );
}

int wh_context_set_alternatives( wh_context* c, int k )
{
	if( !c ) return refuse( "context_set_alternatives: null context" );
	if( k < 0 || k > ALT_MAX_K ) return refuse( "context_set_alternatives: k outside 0 .. 8" );
	if( k == c->altK ) return 0;
	WH_BIND( c->m );
	// a change in mid-window leaves samples of the window without records, or with records of another stride: the window's are no longer read
	c->windowAltK = 0;
	// the switch changes behind the stream: what was queued has run under the k it was queued with
	if( k == 0 ) { WH_HIP( hipStreamSynchronize( c->stream ) ); c->altK = 0; return 0; }
	if( c->hyp != 1 ) return refuse( "context_set_alternatives: not available on a hypothesis-group context (the ring is indexed by the greedy loop's samples)" );
	if( c->flags & WH_FLAG_PARITY_EXACT ) return refuse( "context_set_alternatives: not available under WH_FLAG_PARITY_EXACT" );
	if( c->m->hp.n_vocab > ALT_MAX_VOCAB ) return refuse( "context_set_alternatives: vocabulary larger than 53248" );
	// sized for k = 8 once: a captured step keeps the address
	if( !c->altRing ) WH_CHECK( c->alloc( c->altRing, (int64_t)c->m->hp.n_text_ctx * c->maxSeq * ALT_MAX_K, wh_context::DONT_CARE, "alternatives" ) );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	c->altK = k;
	return 0;
}

// Records of samples [first, first + count) of the window in progress, HOST [count][batch][k]; waits for those samples only, like wh_decode_window_fetch (before
// wh_decode_window_finish, which ends the window).
int wh_decode_window_alternatives( wh_context* c, int first, int count, wh_token_alternative* outHost )
{
	if( !c || !outHost ) return refuse( "decode_window_alternatives: null argument" );
	if( c->windowSamples <= 0 || c->windowAltK <= 0 )
		return refuse( "decode_window_alternatives: no window in progress that was started with wh_context_set_alternatives on and has kept the setting since" );
	if( first < 0 || count <= 0 || first + count > c->windowSamples ) return refuse( "decode_window_alternatives: range not enqueued" );
	WH_BIND( c->m );
	const wh_context::Mark* mk = nullptr;
	for( const auto& x : c->marks )
		if( x.endSample >= first + count ) { mk = &x; break; }
	if( !mk ) return refuse( "decode_window_alternatives: no completion mark for that range" );
	const size_t per = (size_t)c->lastBatch * c->windowAltK;
	if( !c->copyStream ) WH_HIP( hipStreamCreateWithFlags( &c->copyStream, hipStreamNonBlocking ) );
	WH_HIP( hipStreamWaitEvent( c->copyStream, mk->ev, 0 ) );
	WH_HIP( hipMemcpyAsync( outHost, c->altRing + (size_t)first * per, sizeof( TokenAlternative ) * (size_t)count * per, hipMemcpyDeviceToHost, c->copyStream ) );
	WH_HIP( hipStreamSynchronize( c->copyStream ) );
	return 0;
}

}	// extern "C"
