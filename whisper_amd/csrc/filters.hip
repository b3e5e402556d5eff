// The decode-step logit filters and their ONE owner ("The filters' owner"): suppressed tokens, timestamp rules, phrase boosting, no-repeat
// n-grams. Kernels next to the entry points that own their buffers, like align.hip, resample.hip and speech.hip; boost.hip is the host half of phrase boosting.
// All four write c->logits in place between the vocabulary product and the sampler. This unit alone names a member of wh_context::filters; the other units call
// the functions of runtime.h defined below the kernels. A filter added here touches this file, the struct and its setter's declaration -- no other unit.
#include "runtime.h"
#include <algorithm>

namespace wh
{
	namespace
	{
		// ---- suppressed tokens (wh_context_set_suppress; DESIGN.md section 7 "Suppressed tokens") ----------------------
		// logits[ row ][ ids[ i ] ] = -inf for i < count, one workgroup per row: every sampler kernel reads -inf as probability 0, so nothing downstream changes. The
		// count comes from device memory when countDev is non-null (a captured step graph outlives a change of the set) and is held to `cap`, the ids' allocation;
		// an id outside the row is skipped. The ids are ascending, so neighbouring lanes store to ascending addresses of a row the vocabulary product just wrote.
		__global__ void __launch_bounds__( 256 ) suppressLogitsKernel( float* __restrict__ logits, int nVocab, const int* __restrict__ ids, const int* __restrict__ countDev,
			int count, int cap )
		{
			float* const x = logits + (long long)blockIdx.x * nVocab;
			if( countDev ) count = *countDev;
			count = min( count, cap );
			for( int i = threadIdx.x; i < count; i += 256 )
			{
				const int id = ids[ i ];
				if( (unsigned)id < (unsigned)nVocab ) x[ id ] = -INFINITY;
			}
		}

		// ---- timestamp rules (wh_context_set_timestamp_rules; DESIGN.md section 7 "Timestamp rules") ----------------------
		// The three clauses of openai-whisper's ApplyTimestampRules that sampleBest does not hold -- pairs, non-decreasing timestamps, segments of non-zero length --
		// as -inf over ranges of the row, one workgroup per row. The mask depends on what the row has sampled so far: one TimestampRecord per row in device memory.
		// reset 0 (a step of the device-side loop): fold fed[ row ], the previous step's sample, into the record, then mask what the record gives. A record whose
		// count is negative is armed: the fed token is no sample (wh_decode_greedy's first token), nothing is folded and the history starts empty.
		// reset 1 (the prompt step): the record becomes the empty history and nothing is masked -- the first sample is sampleTimestamp( true )'s business. reset 2: armed.
		// Every thread reads the record and the fed token, the barrier follows, and only then thread 0 writes the record back: no lane can see the new one.
		// Plain stores, consecutive lanes to consecutive floats of the row; ranges are held to [0, nVocab).
		__device__ __forceinline__ void fillNegInf( float* __restrict__ x, int lo, int hi )
		{
			for( int i = lo + (int)threadIdx.x; i < hi; i += TSR_THREADS ) x[ i ] = -INFINITY;
		}
		__global__ void __launch_bounds__( TSR_THREADS ) timestampRulesKernel( float* __restrict__ logits, int nVocab, int tokenEot, int tokenBeg, const int* __restrict__ fed,
			int reset, TimestampRecord* __restrict__ records )
		{
			const int row = blockIdx.x;
			if( reset )
			{
				if( threadIdx.x == 0 ) records[ row ] = TimestampRecord{ 0, 0, 0, reset == 2 ? -1 : 0 };
				return;
			}
			TimestampRecord r = records[ row ];
			const int tok = fed[ row ];
			__syncthreads();
			if( r.count < 0 ) r = TimestampRecord{ 0, 0, 0, 0 };
			else
			{
				const int isTs = tok >= tokenBeg ? 1 : 0;
				r.prevTs = r.lastTs;
				r.lastTs = isTs;
				if( isTs ) r.lastId = min( tok, nVocab - 1 );
				r.count = min( r.count + 1, 0x7ffffffe );
			}
			if( threadIdx.x == 0 ) records[ row ] = r;
			float* const x = logits + (long long)row * nVocab;
			// "the one before it" counts as a timestamp while fewer than two tokens have been sampled
			const bool open = r.lastTs && !( r.count < 2 || r.prevTs );	  // text, <|t|>: the pair must close
			if( r.lastTs )
			{
				if( open ) fillNegInf( x, 0, min( tokenEot, nVocab ) );
				else fillNegInf( x, tokenBeg, nVocab );
			}
			// lastId: 0 = no timestamp yet (tokenBeg >= 1). A pair may close at the time it opened; everything else must move on
			if( r.lastId > 0 ) fillNegInf( x, tokenBeg, min( open ? r.lastId : r.lastId + 1, nVocab ) );
		}

		// ---- phrase boosting (wh_context_set_boost; DESIGN.md section 7 "Phrase boosting") ----------------------
		// logits[ row ][ t ] += boost for every token t that continues a phrase after some suffix of what the row has sampled since its last non-text token, one
		// workgroup per row. The suffixes are one state of an Aho-Corasick automaton per row in device memory; the tables (boost.hip) fold the failure chains in, so
		// the step is two searches: delta( n, t ) = n's entry, else the root's, else the root; offered( n ) = n's tokens and the root's.
		// reset 0 (a step of the device-side loop): move the state over fed[ row ], the previous step's sample; an armed state (-1: the fed token is no sample) or a
		// fed id that is no text token gives the root. reset 1 (the prompt step): the root. reset 2: armed. In all three the new state's offers are boosted.
		// Every thread reads the state and the fed token, the barrier follows, and only then thread 0 writes the state back: no lane can see the new one.
		// ONCE per token by construction: a node's tokens are distinct (ascending in the table), and a root token is added only when a search of the node's tokens
		// does not find it -- so no two lanes of the launch store to one float, and plain loads and stores do. The header, the offsets and the nodes read from
		// device memory are held to the limits of a set and every index into the tables to [0, cap): tables and states that are not a compiler's (the idle state a
		// warm-up step runs on) cost wrong floats, never a fault.
		__device__ __forceinline__ int boostLoad( const int* __restrict__ tables, int cap, int i )
		{
			return tables[ min( max( i, 0 ), cap - 1 ) ];
		}
		// the first entry of tok[ lo, hi ) that is not below t, hi when there is none (findEntry of boost.hip)
		__device__ __forceinline__ int boostFind( const int* __restrict__ tables, int cap, int tokBase, int lo, int hi, int t )
		{
			while( lo < hi )
			{
				const int mid = lo + ( ( hi - lo ) >> 1 );
				if( boostLoad( tables, cap, tokBase + mid ) < t ) lo = mid + 1;
				else hi = mid;
			}
			return lo;
		}
		__global__ void __launch_bounds__( BOOST_THREADS ) boostLogitsKernel( float* __restrict__ logits, int nVocab, int tokenEot, const int* __restrict__ tables, int cap,
			const int* __restrict__ fed, int reset, int* __restrict__ states )
		{
			const int row = blockIdx.x;
			const int nodes = min( max( boostLoad( tables, cap, 0 ), 1 ), BOOST_MAX_NODES ), entries = min( max( boostLoad( tables, cap, 1 ), 0 ), BOOST_MAX_ENTRIES );
			const float boost = __int_as_float( boostLoad( tables, cap, 2 ) );
			const BoostTables L = boostTables( nodes, entries );
			const auto span = [ & ]( int n, int& lo, int& hi )
			{
				lo = min( max( boostLoad( tables, cap, L.off + n ), 0 ), entries );
				hi = min( max( boostLoad( tables, cap, L.off + n + 1 ), lo ), entries );
			};
			int rootLo, rootHi;
			span( 0, rootLo, rootHi );
			int state = reset == 2 ? -1 : 0;
			if( !reset )
			{
				const int old = states[ row ];
				const int tok = fed[ row ];
				__syncthreads();
				if( old >= 0 && tok >= 0 && tok < tokenEot )
				{
					int lo, hi;
					span( min( old, nodes - 1 ), lo, hi );
					int e = boostFind( tables, cap, L.tok, lo, hi, tok );
					if( !( e < hi && boostLoad( tables, cap, L.tok + e ) == tok ) )
					{
						e = boostFind( tables, cap, L.tok, rootLo, rootHi, tok );
						if( !( e < rootHi && boostLoad( tables, cap, L.tok + e ) == tok ) ) e = -1;
					}
					state = e < 0 ? 0 : min( max( boostLoad( tables, cap, L.next + e ), 0 ), nodes - 1 );
				}
			}
			if( threadIdx.x == 0 ) states[ row ] = state;
			float* const x = logits + (long long)row * nVocab;
			const int lim = min( tokenEot, nVocab );	  // text tokens only, and inside the row
			const int at = max( state, 0 );
			int lo, hi;
			span( at, lo, hi );
			for( int e = lo + (int)threadIdx.x; e < hi; e += BOOST_THREADS )
			{
				const int t = boostLoad( tables, cap, L.tok + e );
				if( (unsigned)t < (unsigned)lim ) x[ t ] = x[ t ] + boost;
			}
			if( at == 0 ) return;
			for( int e = rootLo + (int)threadIdx.x; e < rootHi; e += BOOST_THREADS )
			{
				const int t = boostLoad( tables, cap, L.tok + e );
				const int mine = boostFind( tables, cap, L.tok, lo, hi, t );
				if( mine < hi && boostLoad( tables, cap, L.tok + mine ) == t ) continue;
				if( (unsigned)t < (unsigned)lim ) x[ t ] = x[ t ] + boost;
			}
		}

		// ---- no-repeat n-grams (wh_context_set_no_repeat; DESIGN.md section 7 "No-repeat n-grams") ----------------------
		// logits[ row ][ t ] = -inf for every text token t (t < tokenEot) that would complete an n-gram the row has already sampled in this window: with h[ 0, L ) the
		// history, every t = h[ i + n - 1 ] whose n - 1 predecessors h[ i, i + n - 1 ) equal the last n - 1 tokens h[ L - n + 1, L ), 0 <= i <= L - n. One workgroup per
		// row; the history is one row of `history` [rows][cap] and one count per row in device memory.
		// reset 0 (a step of the device-side loop): append fed[ row ], the previous step's sample, then mask. A count that is negative is armed: the fed token is no
		// sample (wh_decode_greedy's first token), nothing is appended and the history starts empty. A full history (count == cap) drops the token and masks by what
		// it holds. reset 1 (the prompt step): the history becomes empty and nothing is masked. reset 2: armed.
		// Every thread reads the count and the fed token, the barrier follows, and only then thread 0 writes the token and the count back: no lane can see the new
		// count, and the one history entry that is written in this launch, h[ old count ], is never loaded -- the lanes take it from the register that holds the fed token.
		// Each lane owns start positions i: n - 1 compares against the suffix, which is wave-uniform and kept in registers, then one plain store. The history is
		// under 2 KB per row and every lane reads each entry at most n times through L1 / L2; it is not staged in LDS. Several lanes may find the same t (an n-gram that
		// occurs more than once) and store the same -inf to one float: intended, the result is the same whichever store lands last, as in suppressLogitsKernel with a
		// repeated id. The count, the history entries and the fed id come from device memory: the count is held to [ -1, cap ], positions follow from it and stay inside
		// [ 0, cap ), and a token is used as a column only inside [ 0, min( tokenEot, nVocab ) ). A record that is nobody's history (the idle state a warm-up step runs
		// on) costs wrong floats, never a fault.
		__global__ void __launch_bounds__( NRN_THREADS ) noRepeatKernel( float* __restrict__ logits, int nVocab, int tokenEot, int n, const int* __restrict__ fed, int reset,
			int* __restrict__ history, int* __restrict__ counts, int cap )
		{
			const int row = blockIdx.x;
			if( reset )
			{
				if( threadIdx.x == 0 ) counts[ row ] = reset == 2 ? -1 : 0;
				return;
			}
			const int old = min( counts[ row ], cap );
			const int tok = fed[ row ];
			__syncthreads();
			int* const h = history + (long long)row * cap;
			const bool append = old >= 0 && old < cap;
			const int L = old < 0 ? 0 : append ? old + 1 : cap;
			if( threadIdx.x == 0 )
			{
				if( append ) h[ old ] = tok;
				counts[ row ] = L;
			}
			if( L < n ) return;
			const auto at = [ & ]( int j ) { return ( append && j == old ) ? tok : h[ j ]; };
			int suffix[ NRN_MAX_N - 1 ];
#pragma unroll
			for( int k = 0; k < NRN_MAX_N - 1; k++ ) suffix[ k ] = k < n - 1 ? at( L - n + 1 + k ) : 0;
			float* const x = logits + (long long)row * nVocab;
			const int lim = min( tokenEot, nVocab );	  // text tokens only, and inside the row
			for( int i = (int)threadIdx.x; i <= L - n; i += NRN_THREADS )
			{
				bool same = true;
#pragma unroll
				for( int k = 0; k < NRN_MAX_N - 1; k++ )
					if( k < n - 1 && same ) same = at( i + k ) == suffix[ k ];
				const int t = at( i + n - 1 );
				if( same && (unsigned)t < (unsigned)lim ) x[ t ] = -INFINITY;
			}
		}
	}	// namespace

	int launchSuppressLogits( float* logits, int rows, int nVocab, const int* ids, const int* countDev, int count, int cap, hipStream_t stream )
	{
		if( !logits || !ids || rows < 1 || nVocab < 1 || count < 0 || cap < 0 ) { setError( "suppressLogits: bad argument" ); return -1; }
		hipLaunchKernelGGL( suppressLogitsKernel, dim3( rows ), dim3( 256 ), 0, stream, logits, nVocab, ids, countDev, count, cap );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchTimestampRules( float* logits, int rows, int nVocab, int tokenEot, int tokenBeg, const int* fed, int reset, TimestampRecord* records, hipStream_t stream )
	{
		if( !logits || !records || ( !reset && !fed ) || rows < 1 || nVocab < 2 || tokenBeg < 1 || tokenBeg >= nVocab || tokenEot < 0 || tokenEot >= tokenBeg || reset < 0 || reset > 2 )
		{
			setError( "timestampRules: bad argument" );
			return -1;
		}
		hipLaunchKernelGGL( timestampRulesKernel, dim3( rows ), dim3( TSR_THREADS ), 0, stream, logits, nVocab, tokenEot, tokenBeg, fed, reset, records );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchBoostLogits( float* logits, int rows, int nVocab, int tokenEot, const int* tables, int tableInts, const int* fed, int reset, int* states, hipStream_t stream )
	{
		if( !logits || !tables || !states || ( !reset && !fed ) || rows < 1 || nVocab < 1 || nVocab > BOOST_MAX_VOCAB || tokenEot < 0 || tokenEot > nVocab || tableInts < 4 || reset < 0 || reset > 2 )
		{
			setError( "boostLogits: bad argument" );
			return -1;
		}
		hipLaunchKernelGGL( boostLogitsKernel, dim3( rows ), dim3( BOOST_THREADS ), 0, stream, logits, nVocab, tokenEot, tables, tableInts, fed, reset, states );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	int launchNoRepeat( float* logits, int rows, int nVocab, int tokenEot, int n, const int* fed, int reset, int* history, int* counts, int cap, hipStream_t stream )
	{
		if( !logits || !history || !counts || ( !reset && !fed ) || rows < 1 || nVocab < 1 || tokenEot < 0 || tokenEot > nVocab || n < 1 || n > NRN_MAX_N || reset < 0 || reset > 2 || cap < 1 )
		{
			setError( "noRepeat: bad argument" );
			return -1;
		}
		hipLaunchKernelGGL( noRepeatKernel, dim3( rows ), dim3( NRN_THREADS ), 0, stream, logits, nVocab, tokenEot, n, fed, reset, history, counts, cap );
		WH_HIP( hipGetLastError() );
		return 0;
	}
}	// namespace wh

// ---- the owner of wh_context::filters ------------------------------------------------------------------------
static int tokenEot( const wh_context* c ) { return specialIds( c->m->hp ).sot - 1; }	  // <|endoftext|>: the end of the text tokens, the only ones a filter touches
static int refuse( const std::string& text ) { setError( text.c_str() ); return WH_E_INVALIDARG; }

// The ONE place suppressed tokens take effect: behind the launch that finishes c->logits, -inf over the set's columns of every row. Every consumer -- wh_decode's
// softmax, the greedy, tempered and per-row samplers, the beam step, the no-speech gather -- reads the filtered row. Stateless: the same mask for every row and
// step, so decodeGraph ends with it on both of its routes. Accounted under the sampler's class, like the three below: timingsPrint's sections are the reference's.
int wh::filterLogits( wh_context* c, int batch )
{
	const LogitFilters& f = c->filters;
	if( f.suppressHeld <= 0 || f.suppressOff ) return 0;
	return profiled( c, KC_SAMPLE, 0.0, 4.0 * batch * f.suppressHeld,
		[ & ]() { return launchSuppressLogits( c->logits, batch, c->m->hp.n_vocab, f.suppressSet + 1, f.suppressSet, 0, tokenEot( c ), c->stream ); } );
}
// set around the one pass that must see the model's own row (wh_lang_detect, like AlignHook around wh_align_tokens); never captured, so no part of a key
void wh::bypassFilterLogits( wh_context* c, bool on ) { c->filters.suppressOff = on; }

// The filters whose effect depends on what each row has sampled: one launch each, right behind decodeGraph -- so behind the suppress launch -- and in front of
// the sampler, reading the fed token c->tokensDev[ row ], the previous step's sample. Only the device-side loop calls this: wh_decode, wh_lang_detect,
// wh_align_tokens and the beam step do not. The order -- rules, boost, n-grams -- does not change the row: the two masks only write -inf, and -inf + boost stays
// -inf. `phase` is the kernels' reset argument (their header comments say what 0, 1 and 2 do). The one asymmetry: FILTER_ARM arms the boost states with a memset
// (-1 in every int), not a launch: a boost launch adds the new state's offers in every phase, and wh_decode_greedy has no row yet -- the first step boosts its own.
int wh::filterLoopRows( wh_context* c, int batch, eFilterPhase phase )
{
	const LogitFilters& f = c->filters;
	const wh_hparams& hp = c->m->hp;
	const int eot = tokenEot( c ), reset = (int)phase;
	if( f.rulesOn )
		WH_CHECK( profiled( c, KC_SAMPLE, 0.0, 4.0 * batch * hp.n_vocab,
			[ & ]() { return launchTimestampRules( c->logits, batch, hp.n_vocab, eot, specialIds( hp ).beg, c->tokensDev, reset, f.ruleRecords, c->stream ); } ) );
	if( f.phrasesOn && phase == FILTER_ARM ) WH_HIP( hipMemsetAsync( f.phraseStates, 0xFF, sizeof( int32_t ) * (size_t)batch, c->stream ) );
	else if( f.phrasesOn )
		WH_CHECK( profiled( c, KC_SAMPLE, 0.0, 8.0 * batch * BOOST_MAX_PHRASES,
			[ & ]() { return launchBoostLogits( c->logits, batch, hp.n_vocab, eot, f.phraseTables, BOOST_TABLE_INTS, c->tokensDev, reset, f.phraseStates, c->stream ); } ) );
	if( f.ngramN )
		WH_CHECK( profiled( c, KC_SAMPLE, 0.0, 4.0 * batch * hp.n_text_ctx,
			[ & ]() { return launchNoRepeat( c->logits, batch, hp.n_vocab, eot, f.ngramN, c->tokensDev, reset, f.ngramHistory, f.ngramCounts, hp.n_text_ctx, c->stream ); } ) );
	return 0;
}

// What the filters add to stepKey (step_graph.hip): one more node in a step's launch sequence each. The ids, records, tables and histories are device memory's.
//   STEP_KEY_SUPPRESS       a suppressed set is held: one more node behind the logits, the same for every set; decodeGraph's, so every kind of step shares it
//   STEP_KEY_TS_RULES       the timestamp rules are on: one more node in front of the sampler, the same for every window
//   STEP_KEY_BOOST          a set of boosted phrases is held: one more node in front of the sampler, the same for every set and boost
//   STEP_KEY_NO_REPEAT * n  no-repeat n-grams are on, n = 1 .. 8 in bits 27-30: one more node there, and n is its kernel's argument, so no graph serves another n
// The last three are the greedy loop's alone: a beam step has no sampler in front of which they would run, and their bits stay clear in its key.
static constexpr uint32_t STEP_KEY_SUPPRESS = 0x80000u, STEP_KEY_TS_RULES = 0x100000u, STEP_KEY_BOOST = 0x4000000u, STEP_KEY_NO_REPEAT = 0x8000000u;
uint32_t wh::filterGraphKey( const wh_context* c ) { return c->filters.suppressHeld > 0 ? STEP_KEY_SUPPRESS : 0u; }
uint32_t wh::filterLoopKey( const wh_context* c )
{
	const LogitFilters& f = c->filters;
	return ( f.rulesOn ? STEP_KEY_TS_RULES : 0u ) | ( f.phrasesOn ? STEP_KEY_BOOST : 0u ) | STEP_KEY_NO_REPEAT * (uint32_t)f.ngramN;
}

// Everything in the filters' device memory that a step of the loop mutates, for `batch` rows: the ONE list of which buffers there are and how big each is,
// handed to `f` in a fixed order. (The suppressed set and the boost tables are read only.)
template<class F> static int eachRowBuffer( const wh_context* c, int batch, F&& f )
{
	const LogitFilters& s = c->filters;
	if( s.rulesOn ) WH_CHECK( f( s.ruleRecords, sizeof( TimestampRecord ) * batch ) );
	if( s.phrasesOn ) WH_CHECK( f( s.phraseStates, sizeof( int32_t ) * batch ) );
	if( s.ngramN ) WH_CHECK( f( s.ngramHistory, sizeof( int32_t ) * batch * c->m->hp.n_text_ctx ) );
	if( s.ngramN ) WH_CHECK( f( s.ngramCounts, sizeof( int32_t ) * batch ) );
	return 0;
}
// The filters' share of LoopState (obtainStepGraph's WARM_PRESERVE; the stream is idle and no setter runs in between): those buffers, one behind the other
int wh::saveFilterState( const wh_context* c, int batch, std::vector<uint8_t>& s )
{
	s.clear();
	const auto read = [ & ]( const void* dev, size_t bytes ) -> int { s.resize( s.size() + bytes ); WH_HIP( hipMemcpy( s.data() + s.size() - bytes, dev, bytes, hipMemcpyDeviceToHost ) ); return 0; };
	return eachRowBuffer( c, batch, read );
}
int wh::restoreFilterState( wh_context* c, int batch, const std::vector<uint8_t>& s )
{
	size_t at = 0;
	const auto write = [ & ]( void* dev, size_t bytes ) -> int { WH_HIP( hipMemcpy( dev, s.data() + at, bytes, hipMemcpyHostToDevice ) ); at += bytes; return 0; };
	return eachRowBuffer( c, batch, write );
}

// Who may turn a filter on, stated once. Not under WH_FLAG_PARITY_EXACT: host-stepped decoding only, no filter launch exists on that route. And, for a filter
// with a state per row (`noun` names it), not on a hypothesis-group context: the beam's reorder moves cache rows between sequences and the state would not follow.
static int mayTurnOn( const wh_context* c, const std::string& setter, const char* noun )
{
	if( noun && c->hyp != 1 ) return refuse( setter + ": not available on a hypothesis-group context (" + noun + " do not follow the beam's reorder)" );
	return ( c->flags & WH_FLAG_PARITY_EXACT ) ? refuse( setter + ": not available under WH_FLAG_PARITY_EXACT" ) : 0;
}
// ... and the same from the other side, for wh_context_set_flags
int wh::filtersAllowFlags( const wh_context* c, uint32_t flags )
{
	const LogitFilters& f = c->filters;
	const char* const held = f.suppressHeld > 0 ? "wh_context_set_suppress holds a set" : f.phrasesOn ? "wh_context_set_boost holds a set" :
		f.ngramN ? "wh_context_set_no_repeat is on" : f.rulesOn ? "wh_context_set_timestamp_rules is on" : nullptr;
	return ( flags & WH_FLAG_PARITY_EXACT ) && held ? refuse( std::string( "context_set_flags: WH_FLAG_PARITY_EXACT is not available while " ) + held ) : 0;
}
// a filter with a state per row changes its switch behind the stream -- a chunk queued earlier has run under the mode it was enqueued in: the off path's wait
static int waitForStream( wh_context* c ) { WH_BIND( c->m ); WH_HIP( hipStreamSynchronize( c->stream ) ); return 0; }

// Suppressed tokens. The sorted unique set and its count go to device memory behind what the stream holds.
extern "C" int wh_context_set_suppress( wh_context* c, const int32_t* ids, int count )
{
	if( !c || count < 0 || ( count > 0 && !ids ) ) return refuse( "context_set_suppress: null context, a negative count or null ids" );
	LogitFilters& f = c->filters;
	const int eot = tokenEot( c );
	for( int i = 0; i < count; i++ )
		if( ids[ i ] < 0 || ids[ i ] >= eot )
			return refuse( "context_set_suppress: id " + std::to_string( ids[ i ] ) + " at index " + std::to_string( i ) + " is outside [0, " + std::to_string( eot ) + "): only text tokens can be suppressed" );
	if( count > 0 ) WH_CHECK( mayTurnOn( c, "context_set_suppress", nullptr ) );
	if( count == 0 && !f.suppressSet ) return 0;
	WH_BIND( c->m );
	std::vector<int32_t> up( 1 );
	up.insert( up.end(), ids, ids + count );
	std::sort( up.begin() + 1, up.end() );
	up.erase( std::unique( up.begin() + 1, up.end() ), up.end() );
	up[ 0 ] = (int32_t)up.size() - 1;
	if( !f.suppressSet ) WH_CHECK( c->alloc( f.suppressSet, (int64_t)eot + 1, wh_context::MUST_BE_ZERO, "suppress" ) );
	WH_HIP( hipMemcpyAsync( f.suppressSet, up.data(), sizeof( int32_t ) * up.size(), hipMemcpyHostToDevice, c->stream ) );
	WH_HIP( hipStreamSynchronize( c->stream ) );	 // `up` is this call's
	f.suppressHeld = up[ 0 ];
	return 0;
}

extern "C" int wh_context_set_timestamp_rules( wh_context* c, int on )
{
	if( !c ) return refuse( "context_set_timestamp_rules: null context" );
	LogitFilters& f = c->filters;
	if( !on ) { if( f.rulesOn ) WH_CHECK( waitForStream( c ) ); f.rulesOn = false; return 0; }
	WH_CHECK( mayTurnOn( c, "context_set_timestamp_rules", "the records" ) );
	WH_BIND( c->m );
	if( !f.ruleRecords ) WH_CHECK( c->alloc( f.ruleRecords, (int64_t)c->maxSeq, wh_context::MUST_BE_ZERO, "tsRecords" ) );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	f.rulesOn = true;
	return 0;
}

// Phrase boosting. The set is compiled on the host (boost.hip) and uploaded behind what the stream holds.
extern "C" int wh_context_set_boost( wh_context* c, const int32_t* tokens, const int32_t* lens, int count, int nMax, float boost )
{
	if( !c || count < 0 ) return refuse( "context_set_boost: null context or a negative count" );
	LogitFilters& f = c->filters;
	if( count == 0 ) { if( f.phrasesOn ) WH_CHECK( waitForStream( c ) ); f.phrasesOn = false; return 0; }
	WH_CHECK( mayTurnOn( c, "context_set_boost", "the states" ) );
	int64_t nInts = 0;
	WH_CHECK( wh_boost_compile( tokens, lens, count, nMax, tokenEot( c ), c->m->hp.n_vocab, boost, nullptr, 0, &nInts ) );
	std::vector<int32_t> up( (size_t)nInts );
	WH_CHECK( wh_boost_compile( tokens, lens, count, nMax, tokenEot( c ), c->m->hp.n_vocab, boost, up.data(), nInts, &nInts ) );
	WH_BIND( c->m );
	if( !f.phraseTables ) WH_CHECK( c->alloc( f.phraseTables, (int64_t)BOOST_TABLE_INTS, wh_context::MUST_BE_ZERO, "boostTables" ) );
	if( !f.phraseStates ) WH_CHECK( c->alloc( f.phraseStates, (int64_t)c->maxSeq, wh_context::MUST_BE_ZERO, "boostStates" ) );
	WH_HIP( hipMemcpyAsync( f.phraseTables, up.data(), sizeof( int32_t ) * up.size(), hipMemcpyHostToDevice, c->stream ) );
	WH_HIP( hipStreamSynchronize( c->stream ) );	 // `up` is this call's
	f.phrasesOn = true;
	return 0;
}

extern "C" int wh_context_set_no_repeat( wh_context* c, int n )
{
	if( !c ) return refuse( "context_set_no_repeat: null context" );
	if( n < 0 || n > NRN_MAX_N ) return refuse( "context_set_no_repeat: n outside 0 .. 8" );
	LogitFilters& f = c->filters;
	if( n == f.ngramN ) return 0;
	if( n == 0 ) { WH_CHECK( waitForStream( c ) ); f.ngramN = 0; return 0; }
	WH_CHECK( mayTurnOn( c, "context_set_no_repeat", "the histories" ) );
	WH_BIND( c->m );
	if( !f.ngramHistory ) WH_CHECK( c->alloc( f.ngramHistory, (int64_t)c->maxSeq * c->m->hp.n_text_ctx, wh_context::MUST_BE_ZERO, "nrnHistory" ) );
	if( !f.ngramCounts ) WH_CHECK( c->alloc( f.ngramCounts, (int64_t)c->maxSeq, wh_context::MUST_BE_ZERO, "nrnCounts" ) );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	f.ngramN = n;
	return 0;
}
