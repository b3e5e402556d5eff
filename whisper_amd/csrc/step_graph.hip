// The ONE owner of captured decode steps. Every decoded token of the device-side loops -- greedy, tempered, per-row (decode.hip) and beam (beam.hip) -- is one replay
// of a hipGraph captured from one eager run of the step. This unit decides whether a call may replay, states what a captured step depends on (the key), keeps the
// graphs (wh_context::stepGraphs) with their retention rule, captures on first use and enqueues. The steps themselves stay with their loops.
#include "runtime.h"

// the three things that forbid a replay: the profiler brackets every launch, the caller asked for eager launches, WH_DEBUG_SYNC waits after every launch
bool wh::stepsReplayable( const wh_context* c )
{
	return !c->prof.on && !( c->flags & WH_FLAG_NO_GRAPH ) && !debugSync();
}

// Everything besides the batch that changes the launch sequence of a step, for every kind of step. Values (temperatures, seeds) live in device memory and are
// no part of it: one graph serves them all.
//   bits 0-15 + 0x10000  WH_FLAG_PARITY_PV and its thread count (other attention kernels)
//   0x20000              a temperature is set (wh_context_set_sampling: other sampler kernels, the same for every temperature)
//   STEP_KEY_ROWS        per-row sampling (wh_context_set_sampling_rows)
//   the logit filters    filterGraphKey / filterLoopKey (filters.hip, where their bits are explained)
//   STEP_KEY_BEAM + width in bits 22-25: a beam step of that width. It runs decodeGraph like the greedy step, so it shares the parity input and filterGraphKey; it
//                        has no sampler and none of the filters in front of one, so the other bits stay clear
uint32_t wh::stepKey( const wh_context* c, int beamWidth )
{
	const uint32_t graph = ( ( c->flags & WH_FLAG_PARITY_PV ) ? ( 0x10000u | (uint32_t)c->parityThreads ) : 0u ) | filterGraphKey( c );
	if( beamWidth > 0 ) return graph | STEP_KEY_BEAM | ( (uint32_t)beamWidth << 22 );
	return graph | ( c->temperature > 0.0f ? 0x20000u : 0u ) | ( c->sampleRowsOn ? STEP_KEY_ROWS : 0u ) | filterLoopKey( c );
}

// Retention, applied when ( batch, key ) is about to be captured. Entries of the other kind stay: a hypothesis-group context may run greedy and beam windows in
// turn. Of the same kind, an entry goes when it differs in the batch or in the key -- except that a greedy entry may differ in the per-row bit: at most the
// greedy graph and the per-row graph of one batch live side by side, so a lock-step batch whose rounds enter and leave the per-row mode never recaptures, and
// there is at most one beam entry. The caller has waited for the stream: a graph that goes may have been queued.
static void dropStaleStepGraphs( wh_context* c, int batch, uint32_t key )
{
	const uint32_t sibling = ( key & STEP_KEY_BEAM ) ? 0u : STEP_KEY_ROWS;
	for( size_t i = 0; i < c->stepGraphs.size(); )
	{
		const wh_context::StepGraph& g = c->stepGraphs[ i ];
		const bool sameKind = ( ( g.key ^ key ) & STEP_KEY_BEAM ) == 0;
		if( sameKind && ( g.batch != batch || ( ( g.key ^ key ) & ~sibling ) != 0 ) )
		{
			(void)hipGraphExecDestroy( g.exec );
			c->stepGraphs.erase( c->stepGraphs.begin() + (ptrdiff_t)i );
		}
		else i++;
	}
}

// One run of `step`, captured on the context's stream and kept under ( batch, key ). A step that fails inside the capture still ends the capture; a failed
// instantiate leaves no entry.
static int captureStepGraph( wh_context* c, int batch, uint32_t key, const StepFn& step, hipGraphExec_t& exec )
{
	hipGraph_t graph = nullptr;
	WH_HIP( hipStreamBeginCapture( c->stream, hipStreamCaptureModeThreadLocal ) );
	const int rc = step();
	const hipError_t e = hipStreamEndCapture( c->stream, &graph );
	if( rc != 0 ) { if( graph ) (void)hipGraphDestroy( graph ); return rc; }
	if( e != hipSuccess ) return hipFail( e, "hipStreamEndCapture", __FILE__, __LINE__ );
	exec = nullptr;
	const hipError_t e2 = hipGraphInstantiate( &exec, graph, nullptr, nullptr, 0 );
	(void)hipGraphDestroy( graph );
	if( e2 != hipSuccess ) { exec = nullptr; return hipFail( e2, "hipGraphInstantiate", __FILE__, __LINE__ ); }
	c->stepGraphs.push_back( wh_context::StepGraph{ batch, key, exec } );
	c->stepCaptures++;
	return 0;
}

// The graph of ( batch, key ): the one kept, or -- blocking, once per context and key -- a new one. Capture does not allow the per-kernel function attributes
// a first launch sets, so one eager warm-up step runs first, and a step WRITES: the sampler state, the positions, the fed tokens, the records, one row of the
// self-attention caches at each sequence's position. Which of two protocols keeps that harmless depends on what the device holds, and the wrong one is silent:
//   WARM_FRESH     no window state exists yet (a window's start). `idle` writes a state in which the step is harmless -- idleLoopState, plus a finished search for
//                  the beam -- and whatever it and the warm-up leave is overwritten by the window's own upload. The warm-up runs at position 0 and writes cache
//                  row 0, which the window's prompt step rewrites.
//   WARM_PRESERVE  state that must survive is on the device: a window continued after a start without steps, or wh_decode_greedy, whose nPast may be above 0
//                  over cache rows of an earlier wh_decode. The warm-up runs where the state stands -- at position 0 it would clobber row 0 of a live cache;
//                  the row it writes instead is the one the first replayed step rewrites -- and everything else the step mutates (LoopState) is read back
//                  before it and rewritten after the capture. `idle` is not called.
int wh::obtainStepGraph( wh_context* c, int batch, uint32_t key, eWarmUp warm, const StepFn& idle, const StepFn& step, hipGraphExec_t& exec )
{
	exec = c->stepGraph( batch, key );
	if( exec ) return 0;
	// a graph that can no longer be replayed may still be queued, and the state read back below must be complete: wait before either
	WH_HIP( hipStreamSynchronize( c->stream ) );
	dropStaleStepGraphs( c, batch, key );
	LoopState saved;
	if( warm == WARM_PRESERVE ) WH_CHECK( saveLoopState( c, batch, saved ) );
	else WH_CHECK( idle() );
	WH_CHECK( step() );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	WH_CHECK( captureStepGraph( c, batch, key, step, exec ) );
	if( warm == WARM_PRESERVE ) WH_CHECK( restoreLoopState( c, batch, saved ) );
	return 0;
}

// The idle state of WARM_FRESH: a zero sampler state, every sequence at position 0 feeding token 0. Blocking copies from this call's memory, not through the
// pinned staging, which may already hold the window's prompt.
int wh::idleLoopState( wh_context* c, int batch )
{
	const DecodeState warm = { 0, 0, 0, 0 };
	const std::vector<int32_t> zeros( (size_t)batch, 0 );
	WH_HIP( hipMemcpy( c->state, &warm, sizeof( warm ), hipMemcpyHostToDevice ) );
	WH_HIP( hipMemcpy( c->seqPos, zeros.data(), sizeof( int32_t ) * batch, hipMemcpyHostToDevice ) );
	WH_HIP( hipMemcpy( c->tokensDev, zeros.data(), sizeof( int32_t ) * batch, hipMemcpyHostToDevice ) );
	return 0;
}

// nSteps steps behind what the stream holds: replays of `exec`, or -- exec == nullptr -- eager runs of `step`, each with the profiler's key count for the
// position it feeds (firstKeys for the first)
int wh::enqueueSteps( wh_context* c, hipGraphExec_t exec, int nSteps, int firstKeys, const StepFn& step )
{
	for( int s = 0; s < nSteps; s++ )
	{
		if( exec ) { WH_HIP( hipGraphLaunch( exec, c->stream ) ); continue; }
		c->profKeysHint = firstKeys + s;
		WH_CHECK( step() );
	}
	return 0;
}

extern "C" int wh_debug_step_captures( wh_context* c, int* count )
{
	if( !c || !count ) { setError( "debug_step_captures: null argument" ); return WH_E_INVALIDARG; }
	*count = c->stepCaptures;
	return 0;
}
