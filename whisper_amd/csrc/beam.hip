// Beam search: the ranking of a step and the cache reorder on the device (their kernels stand next to the entry points that own their state, like those of
// resample.hip, vad.hip, dequant.hip and align.hip), the host-ranked entry points (candidates, cache reorder) and the device-ranked window.
#include "runtime.h"

namespace wh
{
	namespace
	{
		// ---- self-attention cache rows of sequence parents[j] -> sequence j (beam search: hypotheses change lineage) ----
		// Two launches through a scratch copy, so that a permutation (j <- p while p <- q) reads only rows nobody has overwritten:
		// phase 0: scratch[ j ] = cache[ parents[ j ] ], phase 1: cache[ j ] = scratch[ j ]; sequences with parents[ j ] == j are skipped.
		// grid (heads, sequences, layers x 2 (K, V)); rows x 128 bytes per block.
		__global__ void __launch_bounds__( 256 ) reorderCacheKernel( f16* __restrict__ cacheK, f16* __restrict__ cacheV, f16* __restrict__ scratchK,
			f16* __restrict__ scratchV, const int* __restrict__ parents, int heads, int seqStrideSeqs, int keyStride, int rows, int phase,
			const int* __restrict__ rowsDev )
		{
			const int h = blockIdx.x, j = blockIdx.y, l = blockIdx.z >> 1, kv = blockIdx.z & 1;
			const int p = parents[ j ];
			if( p == j ) return;
			// beam search inside a captured graph: the rows that exist are the sequence's decoder position, in device memory
			if( rowsDev ) rows = min( max( rowsDev[ j ], 0 ), keyStride );
			f16* const cache = kv ? cacheV : cacheK;
			f16* const scratch = kv ? scratchV : scratchK;
			const long long layer = (long long)l * seqStrideSeqs * heads * keyStride * HEAD_DIM;
			const f16* src = ( phase == 0 ? cache + layer + ( (long long)p * heads + h ) * keyStride * HEAD_DIM : scratch + layer + ( (long long)j * heads + h ) * keyStride * HEAD_DIM );
			f16* dst = ( phase == 0 ? scratch : cache ) + layer + ( (long long)j * heads + h ) * keyStride * HEAD_DIM;
			for( int i = threadIdx.x; i < rows * 8; i += 256 ) *(f16x8*)( dst + i * 8 ) = *(const f16x8*)( src + i * 8 );
		}

		// The same move for the hypotheses of ONE WINDOW in ONE launch and without the scratch copy (round 6, option reorder_group): the ranking keeps a hypothesis'
		// parent inside its window's group of `group` consecutive sequences, and row r of sequence j depends on row r of its parent only -- so the thread that owns
		// an element position reads that position from every moved sequence's parent into registers and only then writes the moved sequences: no position is written
		// before its last reader has it. Half the bytes of the two-phase copy (no scratch round trip), one launch instead of two. grid (heads, windows, layers x 2).
		template<int GROUP>
		__global__ void __launch_bounds__( 256 ) reorderCacheGroup( f16* __restrict__ cacheK, f16* __restrict__ cacheV, const int* __restrict__ parents, int heads,
			int seqStrideSeqs, int keyStride, const int* __restrict__ rowsDev )
		{
			const int h = blockIdx.x, w = blockIdx.y, l = blockIdx.z >> 1, kv = blockIdx.z & 1;
			const int base = w * GROUP;
			int par[ GROUP ];
			bool any = false;
	#pragma unroll
			for( int j = 0; j < GROUP; j++ )
			{
				int p = parents[ base + j ] - base;
				p = ( p < 0 || p >= GROUP ) ? j : p;	  // (a parent outside the group cannot come from the ranking kernel; such a slot stays as it is)
				par[ j ] = p;
				any = any || p != j;
			}
			if( !any ) return;
			const int rows = min( max( rowsDev[ base ], 0 ), keyStride );	  // the sequences of a window stand at one position
			f16* const cache = ( kv ? cacheV : cacheK ) + (long long)l * seqStrideSeqs * heads * keyStride * HEAD_DIM;
			auto rowsOf = [ & ]( int j ) -> f16* { return cache + ( (long long)( base + j ) * heads + h ) * keyStride * HEAD_DIM; };
			for( int i = threadIdx.x; i < rows * 8; i += 256 )
			{
				f16x8 val[ GROUP ];
	#pragma unroll
				for( int j = 0; j < GROUP; j++ )
					if( par[ j ] != j ) val[ j ] = *(const f16x8*)( rowsOf( par[ j ] ) + i * 8 );
	#pragma unroll
				for( int j = 0; j < GROUP; j++ )
					if( par[ j ] != j ) *(f16x8*)( rowsOf( j ) + i * 8 ) = val[ j ];
			}
		}

		// ---- beam search: the ranking of a step on the device (see kernels.h; the host version it restates: ContextImpl::decodeWindowBeam) ----
		constexpr int BEAM_CHUNK_FRAMES = 3000;	   // CHUNK_FRAMES of host/hostLoop.h
		// WindowScan::feed (host/hostLoop.h = ContextImpl.cpp:597-673) on the state of one hypothesis; true = its window is over
		__device__ __forceinline__ bool beamFeed( BeamHyp& h, const BeamRules& r, int id )
		{
			if( r.forced ) { h.nTok++; h.i++; return false; }
			if( h.over ) return true;
			if( id > r.tokenBeg )
			{
				// a timestamp token moves the sliding window; going back in time ends the window (the token is not kept)
				const int seekDeltaNew = 2 * ( id - r.tokenBeg );
				if( h.hasTs && h.seekDelta > seekDeltaNew && h.resultLen < h.i ) { h.over = 1; return true; }
				h.seekDelta = seekDeltaNew;
				h.resultLen = h.i + 1;
				h.hasTs = 1;
			}
			h.nTok++;
			const bool endOfAudio = h.hasTs && r.seek + h.seekDelta + 100 >= r.seekEnd;
			if( id == r.tokenEot || ( r.maxTokens > 0 && h.i >= r.maxTokens ) || endOfAudio )
			{
				if( h.resultLen == 0 )
				{
					if( r.seek + h.seekDelta + 100 >= r.seekEnd )
						h.resultLen = h.i + 1;
					else
					{
						h.failed = 1; h.over = 1;
						return true;
					}
				}
				if( r.singleSegment )
				{
					h.resultLen = h.i + 1;
					h.seekDelta = BEAM_CHUNK_FRAMES;
				}
				h.over = 1;
				return true;
			}
			// stuck in a repetition loop: give up on this window
			if( h.i == r.nMax - 1 && ( h.resultLen == 0 || h.seekDelta < BEAM_CHUNK_FRAMES / 2 ) )
			{
				h.failed = 1; h.over = 1;
				return true;
			}
			h.i++;
			if( h.i >= r.nMax ) h.over = 1;
			return h.over != 0;
		}
		__device__ __forceinline__ double beamPerToken( const BeamHyp& h ) { return h.sum / (double)max( 1, h.nTok ); }

		// The ranking of one window by ONE lane: S, cand (the window's slots x width proposals) and logP live in LDS (the kernel below stages them: a lane walking its
		// state in global memory paid a dependent round trip per field, 48 us per step)
		struct BeamProp { int parent, k; double score; };
		// lane 0's working arrays: in LDS as well (private arrays indexed at run time are scratch memory -- a memory round trip per element of the insertion sort)
		struct BeamRankWork
		{
			BeamProp pool[ BEAM_MAX_WIDTH * BEAM_MAX_WIDTH ];
			BeamHyp newLive[ BEAM_MAX_WIDTH ];
			int parentSlot[ BEAM_MAX_WIDTH ], lastTok[ BEAM_MAX_WIDTH ];
		};
		__device__ __forceinline__ void beamRankWindow( BeamWindow& S, BeamRankWork& W, const TokenData* cand, const double* logP, int w, int slots, int width, const BeamRules* __restrict__ rules,
			BeamRecord* __restrict__ records, int maxSteps, int windows, int* __restrict__ parents, int* __restrict__ nextTokens )
		{
			const int base = w * slots;
			if( S.done || S.step >= maxSteps )
			{
				// nothing moves any more: every slot continues itself (the reorder skips it) and feeds its last token again
				for( int b = 0; b < slots; b++ ) parents[ base + b ] = base + b;
				S.done = 1;
				return;
			}
			const BeamRules R = rules[ w ];
			const int step = S.step;
			const bool first = step == 0;
			// ---- the pool: (parent, candidate) with parent score + log p, ranked; ties keep the parent's order, then the candidate's ----
			typedef BeamProp Prop;
			Prop* const pool = W.pool;
			int nPool = 0;
			const int nParents = first ? 1 : S.nLive;	   // the first sample: every slot holds the same prompt, slot 0 speaks for all
			for( int i = 0; i < nParents; i++ )
				for( int k = 0; k < width; k++ )
				{
					const double lp = logP[ i * width + k ];
					pool[ nPool++ ] = Prop{ i, k, ( first ? 0.0 : S.live[ i ].sum ) + lp };
				}
			for( int a = 1; a < nPool; a++ )	   // stable insertion sort, descending score
			{
				const Prop x = pool[ a ];
				int b = a - 1;
				while( b >= 0 && pool[ b ].score < x.score ) { pool[ b + 1 ] = pool[ b ]; b--; }
				pool[ b + 1 ] = x;
			}
			// ---- the best `width` proposals continue their parents: live or, when the stop rules end the window, finished ----
			BeamHyp* const newLive = W.newLive;
			int* const parentSlot = W.parentSlot;
			int* const lastTok = W.lastTok;
			int nNew = 0, accepted = 0;
			BeamRecord* const rec = records + ( (long long)step * windows + w ) * width;
			for( int q = 0; q < nPool && accepted < width; q++ )
			{
				const Prop pr = pool[ q ];
				const TokenData t = cand[ pr.parent * width + pr.k ];
				BeamHyp h;
				if( first )
				{
					h.sum = 0.0; h.i = 0; h.hasTs = 0; h.seekDelta = BEAM_CHUNK_FRAMES; h.resultLen = 0; h.failed = 0; h.over = 0; h.nTok = 0; h.rec = -1;
				}
				else
					h = S.live[ pr.parent ];
				const int parentRec = h.rec;
				h.sum = pr.score;
				const bool over = beamFeed( h, R, t.id );
				h.rec = step * width + accepted;
				rec[ accepted ] = BeamRecord{ t, parentRec, over ? 1 : 0, 0 };
				accepted++;
				if( over )
				{
					if( S.nFinished < BEAM_MAX_FINISHED ) S.finished[ S.nFinished++ ] = h;
				}
				else
				{
					parentSlot[ nNew ] = pr.parent;
					lastTok[ nNew ] = t.id;
					newLive[ nNew++ ] = h;
				}
			}
			for( int a = accepted; a < width; a++ ) rec[ a ] = BeamRecord{ TokenData{ 0, 0, 0.0f, 0.0f, 0.0f }, -2, 0, 0 };	   // unused entries of the step
			for( int i = 0; i < nNew; i++ ) S.live[ i ] = newLive[ i ];
			S.nLive = nNew;
			S.step = step + 1;
			// ---- does a live hypothesis still have a chance? (a cumulative log-probability only ever decreases) ----
			bool keep = nNew > 0;
			if( keep && S.nFinished >= width )
			{
				double bestFinished = -1e300, bestLive = -1e300;
				for( int i = 0; i < S.nFinished; i++ )
					if( !S.finished[ i ].failed ) bestFinished = fmax( bestFinished, S.finished[ i ].sum );
				for( int i = 0; i < nNew; i++ ) bestLive = fmax( bestLive, S.live[ i ].sum );
				keep = bestLive >= bestFinished;
			}
			if( keep && S.nFinished > 2 * width )
			{
				// the finished list keeps its best `width` entries: successful windows first, then log-probability per token (stable)
				for( int a = 1; a < S.nFinished; a++ )
				{
					const BeamHyp x = S.finished[ a ];
					int b = a - 1;
					while( b >= 0 )
					{
						const BeamHyp& y = S.finished[ b ];
						const bool xFirst = x.failed != y.failed ? !x.failed : beamPerToken( x ) > beamPerToken( y );
						if( !xFirst ) break;
						S.finished[ b + 1 ] = y;
						b--;
					}
					S.finished[ b + 1 ] = x;
				}
				S.nFinished = width;
			}
			// the context's end (WindowScan's own bound fires first for every prompt the host loop builds)
			if( keep && S.nPrompt + ( S.step - 1 ) >= S.nTextCtx ) keep = false;
			if( !keep )
			{
				S.done = 1;
				for( int b = 0; b < slots; b++ ) parents[ base + b ] = base + b;
				return;
			}
			// live hypothesis j decodes in slot j next: its cache rows come from its parent's slot; idle slots repeat hypothesis 0 and are ignored
			for( int b = 0; b < slots; b++ )
			{
				const int j = b < nNew ? b : 0;
				parents[ base + b ] = base + parentSlot[ j ];
				nextTokens[ base + b ] = lastTok[ j ];
			}
		}

		// One workgroup per window: 64 lanes stage the window's state, proposals and their log-probabilities (a double-precision log is ~1 us on a single lane) in LDS,
		// lane 0 ranks and runs the state machines, 64 lanes write the state back.
		__global__ void __launch_bounds__( 64 ) beamRankKernel( const TokenData* __restrict__ cand, int slots, int width, const BeamRules* __restrict__ rules,
			BeamWindow* __restrict__ state, BeamRecord* __restrict__ records, int maxSteps, int windows, int* __restrict__ parents, int* __restrict__ nextTokens )
		{
			const int w = blockIdx.x;
			__shared__ BeamWindow S;
			__shared__ TokenData candS[ BEAM_MAX_WIDTH * BEAM_MAX_WIDTH ];
			__shared__ double logP[ BEAM_MAX_WIDTH * BEAM_MAX_WIDTH ];
			__shared__ BeamRankWork work;
			static_assert( sizeof( BeamWindow ) % 4 == 0, "staged as 32-bit words" );
			constexpr int nWords = (int)( sizeof( BeamWindow ) / 4 );
			int* const sw = (int*)&S;
			int* const gw = (int*)&state[ w ];
			for( int i = threadIdx.x; i < nWords; i += 64 ) sw[ i ] = gw[ i ];
			if( (int)threadIdx.x < slots * width )
			{
				const TokenData t = cand[ (long long)w * slots * width + threadIdx.x ];
				candS[ threadIdx.x ] = t;
				logP[ threadIdx.x ] = log( fmax( (double)t.p, 1e-30 ) );
			}
			__syncthreads();
			if( threadIdx.x == 0 ) beamRankWindow( S, work, candS, logP, w, slots, width, rules, records, maxSteps, windows, parents, nextTokens );
			__syncthreads();
			for( int i = threadIdx.x; i < nWords; i += 64 ) gw[ i ] = sw[ i ];
		}
	}	// namespace

	int launchReorderCache( f16* cacheK, f16* cacheV, f16* scratchK, f16* scratchV, const int* parents, int layers, int sequences, int maxSeq,
		int heads, int keyStride, int rows, hipStream_t stream )
	{
		for( int phase = 0; phase < 2; phase++ )
		{
			hipLaunchKernelGGL( reorderCacheKernel, dim3( heads, sequences, layers * 2 ), dim3( 256 ), 0, stream, cacheK, cacheV, scratchK, scratchV, parents,
				heads, maxSeq, keyStride, rows, phase, (const int*)nullptr );
			WH_HIP( hipGetLastError() );
		}
		return 0;
	}

	int launchReorderCacheDev( f16* cacheK, f16* cacheV, f16* scratchK, f16* scratchV, const int* parents, const int* rowsDev, int layers, int sequences, int maxSeq,
		int heads, int keyStride, int group, hipStream_t stream )
	{
		// option reorder_group: the hypotheses of a window move inside their group, in one launch through registers
		if( g_opt.reorderGroup && rowsDev && group > 1 && ( sequences % group ) == 0 )
		{
			const dim3 grid( heads, sequences / group, layers * 2 );
			switch( group )
			{
	#define WH_RG( G ) case G: hipLaunchKernelGGL( reorderCacheGroup<G>, grid, dim3( 256 ), 0, stream, cacheK, cacheV, parents, heads, maxSeq, keyStride, rowsDev ); WH_HIP( hipGetLastError() ); return 0;
				WH_RG( 2 ) WH_RG( 3 ) WH_RG( 4 ) WH_RG( 5 ) WH_RG( 6 ) WH_RG( 7 ) WH_RG( 8 )
	#undef WH_RG
			}
		}
		for( int phase = 0; phase < 2; phase++ )
		{
			hipLaunchKernelGGL( reorderCacheKernel, dim3( heads, sequences, layers * 2 ), dim3( 256 ), 0, stream, cacheK, cacheV, scratchK, scratchV, parents,
				heads, maxSeq, keyStride, 0, phase, rowsDev );
			WH_HIP( hipGetLastError() );
		}
		return 0;
	}

	int launchBeamRank( const TokenData* cand, int windows, int slots, int width, const BeamRules* rules, BeamWindow* state, BeamRecord* records, int maxSteps,
		int* parents, int* nextTokens, hipStream_t stream )
	{
		if( width < 1 || width > BEAM_MAX_WIDTH || slots < width || slots > BEAM_MAX_WIDTH || windows <= 0 ) { setError( "beamRank: 1 <= width <= slots <= 8" ); return -1; }
		hipLaunchKernelGGL( beamRankKernel, dim3( windows ), dim3( 64 ), 0, stream, cand, slots, width, rules, state, records, maxSteps, windows, parents, nextTokens );
		WH_HIP( hipGetLastError() );
		return 0;
	}
}	// namespace wh

extern "C" {

int wh_sample_best( wh_context* c, int batch, int forceTimestamp, int isInitial, wh_token_data* out )
{
	if( !c || !out || batch <= 0 || batch > c->maxSeq ) { setError( "sample_best: bad argument" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	const wh_hparams& hp = c->m->hp;
	const SpecialIds sp = specialIds( hp );
	const int sot = sp.sot, solm = sp.solm, tnot = sp.tnot, beg = sp.beg;
	WH_CHECK( profiled( c, KC_SAMPLE, 0.0, 5.0 * 4.0 * batch * hp.n_vocab,
		[ & ]() { return launchSampleBest( c->probs, batch, hp.n_vocab, beg, sot, solm, tnot, forceTimestamp, isInitial, c->tokDataDev, c->stream ); } ) );
	static_assert( sizeof( wh_token_data ) == sizeof( TokenData ), "token data layout" );
	WH_HIP( hipMemcpyAsync( out, c->tokDataDev, sizeof( TokenData ) * batch, hipMemcpyDeviceToHost, c->stream ) );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	return 0;
}

// The first-use buffers of the ranking steps, allocated before any capture: the candidates, and the copy a cache reorder goes through
static int beamCandidateBuffer( wh_context* c )
{
	return c->grow( c->beamCand, (int64_t)c->maxSeq * 8, wh_context::DONT_CARE, "beamCand" );
}
static int reorderScratch( wh_context* c )
{
	const wh_hparams& hp = c->m->hp;
	const int64_t n = (int64_t)hp.n_text_layer * c->maxSeq * hp.n_text_ctx * hp.n_text_state;
	WH_CHECK( c->grow( c->selfKScratch, n, wh_context::DONT_CARE, "selfKScratch" ) );
	return c->grow( c->selfVScratch, n, wh_context::DONT_CARE, "selfVScratch" );
}

int wh_beam_candidates( wh_context* c, int batch, int width, int forceTimestamp, int isInitial, wh_token_data* out )
{
	if( !c || !out || batch <= 0 || batch > c->maxSeq || width < 1 || width > 8 ) { setError( "beam_candidates: bad argument" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	const wh_hparams& hp = c->m->hp;
	const SpecialIds sp = specialIds( hp );
	WH_CHECK( beamCandidateBuffer( c ) );
	WH_CHECK( profiled( c, KC_SAMPLE, 0.0, ( 4.0 + width ) * 4.0 * batch * hp.n_vocab,
		[ & ]() { return launchBeamCandidates( c->probs, batch, hp.n_vocab, sp.beg, sp.sot, sp.solm, sp.tnot, forceTimestamp, isInitial, width, c->beamCand, c->stream ); } ) );
	WH_HIP( hipMemcpyAsync( out, c->beamCand, sizeof( TokenData ) * (size_t)batch * width, hipMemcpyDeviceToHost, c->stream ) );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	return 0;
}

int wh_reorder_self_cache( wh_context* c, int batch, const int32_t* parents, int rows )
{
	if( !c || !parents || batch <= 0 || batch > c->maxSeq || rows < 0 ) { setError( "reorder_self_cache: bad argument" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	const wh_hparams& hp = c->m->hp;
	if( rows > hp.n_text_ctx ) { setError( "reorder_self_cache: more rows than n_text_ctx" ); return WH_E_BOUNDS; }
	bool any = false;
	for( int j = 0; j < batch; j++ )
	{
		if( parents[ j ] < 0 || parents[ j ] >= batch ) { setError( "reorder_self_cache: a parent is outside the batch" ); return WH_E_INVALIDARG; }
		any = any || parents[ j ] != j;
	}
	if( !any || rows == 0 ) return 0;
	WH_CHECK( reorderScratch( c ) );
	WH_HIP( hipStreamSynchronize( c->stream ) );	   // the staging below may still be read by an earlier enqueue
	int32_t* const st = c->pinned + wh_context::PIN_POS;
	for( int j = 0; j < batch; j++ ) st[ j ] = parents[ j ];
	WH_HIP( hipMemcpyAsync( c->tokDataDev, st, sizeof( int32_t ) * batch, hipMemcpyHostToDevice, c->stream ) );	  // tokDataDev: [maxSeq] records of 20 bytes, free between samples
	return profiled( c, KC_EMBED, 0.0, 4.0 * 2.0 * 2.0 * rows * hp.n_text_state * hp.n_text_layer * batch,
		[ & ]() { return launchReorderCache( c->selfK, c->selfV, c->selfKScratch, c->selfVScratch, (const int*)c->tokDataDev, hp.n_text_layer, batch, c->maxSeq,
			hp.n_text_head, hp.n_text_ctx, rows, c->stream ); } );
}

// ---- beam search with the ranking on the device: no host round trip between the steps of a window ----
static int beamBuffers( wh_context* c )
{
	const wh_hparams& hp = c->m->hp;
	WH_CHECK( beamCandidateBuffer( c ) );
	WH_CHECK( reorderScratch( c ) );
	WH_CHECK( c->grow( c->beamRules, c->maxBatch, wh_context::MUST_BE_ZERO, "beamRules" ) );
	WH_CHECK( c->grow( c->beamState, c->maxBatch, wh_context::MUST_BE_ZERO, "beamState" ) );
	WH_CHECK( c->grow( c->beamRecords, (int64_t)hp.n_text_ctx * c->maxBatch * BEAM_MAX_WIDTH, wh_context::DONT_CARE, "beamRecords" ) );
	WH_CHECK( c->grow( c->beamParents, c->maxSeq, wh_context::MUST_BE_ZERO, "beamParents" ) );
	return 0;
}

// one step: parents' cache rows move -> every slot decodes its token -> probabilities -> candidates -> ranking (writes the next step's parents and tokens)
static int beamStep( wh_context* c, int batch, int width )
{
	const wh_hparams& hp = c->m->hp;
	const SpecialIds sp = specialIds( hp );
	hipStream_t st = c->stream;
	WH_CHECK( profiled( c, KC_EMBED, 0.0, 4.0 * 2.0 * 2.0 * c->profKeysHint * hp.n_text_state * hp.n_text_layer * batch,
		[ & ]() { return launchReorderCacheDev( c->selfK, c->selfV, c->selfKScratch, c->selfVScratch, c->beamParents, c->seqPos, hp.n_text_layer, batch, c->maxSeq,
			hp.n_text_head, hp.n_text_ctx, c->hyp, st ); } ) );
	WH_CHECK( decodeGraph( c, batch, 1, 0, true ) );
	WH_CHECK( profiled( c, KC_SOFTMAX, 10.0 * batch * hp.n_vocab, 12.0 * batch * hp.n_vocab, [ & ]() { return launchVocabSoftMax( c->logits, c->probs, batch, hp.n_vocab, st ); } ) );
	WH_CHECK( profiled( c, KC_SAMPLE, 0.0, ( 4.0 + width ) * 4.0 * batch * hp.n_vocab,
		[ & ]() { return launchBeamCandidates( c->probs, batch, hp.n_vocab, sp.beg, sp.sot, sp.solm, sp.tnot, 0, 0, width, c->beamCand, st ); } ) );
	WH_CHECK( profiled( c, KC_SAMPLE, 0.0, 0.0, [ & ]() { return launchBeamRank( c->beamCand, batch / c->hyp, c->hyp, width, c->beamRules, c->beamState, c->beamRecords,
		hp.n_text_ctx, c->beamParents, c->tokensDev, st ); } ) );
	return launchAdvanceState( c->state, c->seqPos, batch, st );
}

// nSteps steps of the window in progress: replays of `exec`, eager launches when there is none
static int beamEnqueue( wh_context* c, hipGraphExec_t exec, int nSteps )
{
	const int batch = c->beamWindows * c->hyp, width = c->beamWidth;
	WH_CHECK( enqueueSteps( c, exec, nSteps, c->windowPos + 1, [ c, batch, width ]() { return beamStep( c, batch, width ); } ) );
	c->beamSteps += nSteps;
	c->windowPos += nSteps;
	return 0;
}

int wh_beam_window_start( wh_context* c, int windows, const int32_t* promptTokens, int nPrompt, int width, const wh_beam_rules* rules, int nSteps )
{
	if( !c || !promptTokens || !rules || windows <= 0 || windows > c->maxBatch || nPrompt <= 0 || nSteps < 0 || width < 1 || width > c->hyp || width > BEAM_MAX_WIDTH )
	{
		setError( "beam_window_start: bad argument (1 <= width <= hypotheses per window of the context <= 8)" );
		return WH_E_INVALIDARG;
	}
	if( !c->encoded ) { setError( "beam_window_start: wh_encode has not run" ); return WH_E_NOT_READY; }
	WH_BIND( c->m );
	const wh_hparams& hp = c->m->hp;
	const int batch = windows * c->hyp;
	if( nPrompt + nSteps > hp.n_text_ctx || (int64_t)batch * nPrompt > c->pinTokenCap() ) { setError( "beam_window_start: too many tokens" ); return WH_E_BOUNDS; }
	static_assert( sizeof( wh_beam_rules ) == sizeof( BeamRules ) && sizeof( wh_beam_window ) == sizeof( BeamWindow ) && sizeof( wh_beam_record ) == sizeof( BeamRecord ) &&
		sizeof( wh_beam_hyp ) == sizeof( BeamHyp ), "beam structure layouts" );
	WH_CHECK( beamBuffers( c ) );
	hipStream_t st = c->stream;
	WH_HIP( hipStreamSynchronize( st ) );	   // the staging and the search state may still be read by an earlier window
	const SpecialIds sp = specialIds( hp );
	c->beamWindows = windows;
	c->beamWidth = width;
	c->beamSteps = 0;
	hipGraphExec_t exec = nullptr;
	if( stepsReplayable( c ) )
	{
		// no window state exists yet. The idle state of a beam step: idleLoopState, a finished search (the ranking returns at once), parents = identity and the
		// rules; what it and the warm-up leave behind is overwritten below. The launch sequence of a step is the same for every token: positions, parents,
		// tokens and the search state live in device memory.
		const StepFn idle = [ c, windows, batch, rules ]()
		{
			std::vector<BeamWindow> idleSearch( (size_t)windows );
			memset( idleSearch.data(), 0, idleSearch.size() * sizeof( BeamWindow ) );
			for( BeamWindow& w : idleSearch ) w.done = 1;
			std::vector<int32_t> ident( (size_t)batch );
			for( int b = 0; b < batch; b++ ) ident[ (size_t)b ] = b;
			WH_HIP( hipMemcpy( c->beamState, idleSearch.data(), idleSearch.size() * sizeof( BeamWindow ), hipMemcpyHostToDevice ) );
			WH_HIP( hipMemcpy( c->beamRules, rules, sizeof( BeamRules ) * windows, hipMemcpyHostToDevice ) );
			WH_HIP( hipMemcpy( c->beamParents, ident.data(), sizeof( int32_t ) * batch, hipMemcpyHostToDevice ) );
			return idleLoopState( c, batch );
		};
		WH_CHECK( obtainStepGraph( c, batch, stepKey( c, width ), WARM_FRESH, idle, [ c, batch, width ]() { return beamStep( c, batch, width ); }, exec ) );
	}
	// the window's own state: rules, an empty search, the prompt of every slot, positions
	{
		std::vector<BeamWindow> init( (size_t)windows );
		memset( init.data(), 0, init.size() * sizeof( BeamWindow ) );
		for( BeamWindow& w : init ) { w.nPrompt = nPrompt; w.nTextCtx = hp.n_text_ctx; }
		WH_HIP( hipMemcpy( c->beamState, init.data(), init.size() * sizeof( BeamWindow ), hipMemcpyHostToDevice ) );
		WH_HIP( hipMemcpy( c->beamRules, rules, sizeof( BeamRules ) * windows, hipMemcpyHostToDevice ) );
	}
	int32_t* const stTok = c->pinTokens();
	const int M = batch * nPrompt;
	for( int w = 0; w < windows; w++ )
	{
		WH_CHECK( checkTokens( hp, promptTokens + (size_t)w * nPrompt, nPrompt, "beam_window_start" ) );
		for( int j = 0; j < c->hyp; j++ )
			for( int i = 0; i < nPrompt; i++ ) stTok[ ( (size_t)w * c->hyp + j ) * nPrompt + i ] = promptTokens[ (size_t)w * nPrompt + i ];
	}
	const DecodeState s0 = { 0, 0, 0, 0 };
	WH_CHECK( uploadDecodeState( c, batch, s0, nullptr, nPrompt ) );	   // after the prompt step every slot stands at position nPrompt
	WH_HIP( hipMemcpyAsync( c->tokensDev, stTok, sizeof( int32_t ) * M, hipMemcpyHostToDevice, st ) );
	WH_CHECK( decodeGraph( c, batch, nPrompt, 0, false ) );
	WH_CHECK( profiled( c, KC_SOFTMAX, 10.0 * batch * hp.n_vocab, 12.0 * batch * hp.n_vocab, [ & ]() { return launchVocabSoftMax( c->logits, c->probs, batch, hp.n_vocab, st ); } ) );
	// the first sample of a window: the reference's sampleTimestamp( true ) rules (forced timestamp, the 1.00 s cap)
	WH_CHECK( profiled( c, KC_SAMPLE, 0.0, ( 4.0 + width ) * 4.0 * batch * hp.n_vocab,
		[ & ]() { return launchBeamCandidates( c->probs, batch, hp.n_vocab, sp.beg, sp.sot, sp.solm, sp.tnot, 1, 1, width, c->beamCand, st ); } ) );
	WH_CHECK( profiled( c, KC_SAMPLE, 0.0, 0.0, [ & ]() { return launchBeamRank( c->beamCand, windows, c->hyp, width, c->beamRules, c->beamState, c->beamRecords, hp.n_text_ctx,
		c->beamParents, c->tokensDev, st ); } ) );
	c->beamSteps = 1;
	c->windowPos = nPrompt;
	c->lastBatch = batch;
	return beamEnqueue( c, exec, nSteps );
}

int wh_beam_window_continue( wh_context* c, int nSteps )
{
	if( !c || nSteps <= 0 || c->beamSteps <= 0 ) { setError( "beam_window_continue: no window in progress" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	if( c->windowPos + nSteps > c->m->hp.n_text_ctx ) { setError( "beam_window_continue: n_text_ctx exceeded" ); return WH_E_BOUNDS; }
	// the graph wh_beam_window_start captured for this shape and mode, when a replay is allowed and it is still there
	return beamEnqueue( c, stepsReplayable( c ) ? c->stepGraph( c->beamWindows * c->hyp, stepKey( c, c->beamWidth ) ) : nullptr, nSteps );
}

int wh_beam_window_status( wh_context* c, wh_beam_window* out )
{
	if( !c || !out || c->beamSteps <= 0 ) { setError( "beam_window_status: no window in progress" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	WH_HIP( hipMemcpyAsync( out, c->beamState, sizeof( BeamWindow ) * (size_t)c->beamWindows, hipMemcpyDeviceToHost, c->stream ) );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	return 0;
}

int wh_beam_window_records( wh_context* c, int firstStep, int count, wh_beam_record* out )
{
	if( !c || !out || firstStep < 0 || count <= 0 || firstStep + count > c->beamSteps ) { setError( "beam_window_records: steps outside what was enqueued" ); return WH_E_BOUNDS; }
	WH_BIND( c->m );
	// device layout [step][windows of the call][width]
	const size_t perStep = (size_t)c->beamWindows * c->beamWidth;
	WH_HIP( hipMemcpyAsync( out, c->beamRecords + (size_t)firstStep * perStep, sizeof( BeamRecord ) * perStep * count, hipMemcpyDeviceToHost, c->stream ) );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	return 0;
}

}	// extern "C"
