// tests/phrase_boost_cpu/batch_driver.cpp -- CPU test harness for phrase boosting in the lock-step batch scheduler (not part of the product).
// One translation unit = the test double of the compute layer (tests/hostloop_cpu/fake_device.cpp) and the batch harness (batch_driver.cpp), both UNCHANGED,
// next to whisper_amd/host/batchScheduler.cpp, plus
//   * the hook the scheduler gets injected (batchBoost.h g_batchBoost): it RECORDS every call -- which context, in which run, how many window starts that
//     context had seen, the set's size, its first token and the boost -- and boosts nothing (the double has no logits), so the transcripts must be those of a
//     runner on which nothing was set;
//   * pb_run: bt_run with a script of changes, one entry applied before each of the runs of ONE runner.
#include "../hostloop_cpu/fake_device.cpp"
#include "../hostloop_cpu/batch_driver.cpp"
#include "batchBoost.h"
#include <map>

namespace Whisper
{
	HRESULT setBatchBoostedPhrases( iBatchRunner* runner, const sBoostedPhrases* phrases );	 // batchScheduler.cpp
}

namespace
{
	struct BoostCall { int context, run, starts, count, first; float boost; };
	std::vector<BoostCall> g_calls;
	std::map<wh_context*, int> g_boostContexts;
	int g_run = 0;
	std::string g_pbOut;

	int hookBoost( wh_context* c, const int32_t* tokens, const int32_t* lens, int count, int nMax, float boost )
	{
		if( !c || ( count > 0 && ( !tokens || !lens || nMax < 1 ) ) ) return WH_E_INVALIDARG;
		if( !g_boostContexts.count( c ) ) { const int id = (int)g_boostContexts.size(); g_boostContexts[ c ] = id; }
		g_calls.push_back( BoostCall{ g_boostContexts[ c ], g_run, c->starts, count, count > 0 ? tokens[ 0 ] : -1, boost } );
		return 0;
	}

	// the two sets of the script: A = { [1000, 1001], [1002] } at 2.5, B = { [1003] } at 4
	HRESULT setA( iBatchRunner* r )
	{
		const int32_t tokens[ 4 ] = { 1000, 1001, 1002, 0 }, lens[ 2 ] = { 2, 1 };
		const sBoostedPhrases p{ tokens, lens, 2, 2, 2.5f };
		return setBatchBoostedPhrases( r, &p );
	}
	HRESULT setB( iBatchRunner* r )
	{
		const int32_t token = 1003, len = 1;
		const sBoostedPhrases p{ &token, &len, 1, 1, 4.0f };
		return setBatchBoostedPhrases( r, &p );
	}
}

extern "C" __attribute__( ( visibility( "default" ) ) ) void pb_install_hook( int install ) { Whisper::g_batchBoost = install ? &hookBoost : nullptr; }

// bt_run's arguments, then a script: before run r (r = 0 .. nRuns - 1) script[ r ] is applied: -1 = no call, 0 = setBatchBoostedPhrases( nullptr ), 1 = set A,
// 2 = set A and then clear, 3 = set A twice, 4 = set B, 5 = a set of count 0, 6 = a set with an id equal to eot (refused). Returns the last run's HRESULT, or the
// HRESULT of setBatchBoostedPhrases when that fails (pb_result() then is "{}").
// pb_result() = bt_result's streams of the last run, "calls":[{"context","run","starts","count","first","boost"}] and "counters": fake_device_counters while the
// runner is alive.
extern "C" __attribute__( ( visibility( "default" ) ) ) int pb_run( const char* modelPath, int rules, uint32_t flags, uint32_t language, int nMaxTextCtx,
	const int32_t* promptTokens, int nPrompt, const float* const* pcm, const int32_t* nSamples, int nBuffers, const BatchStreamDesc* streams, int nStreams,
	uint32_t maxSlots, uint32_t groups, uint32_t chunk, uint32_t lookahead, int threads, const int32_t* script, int nRuns )
{
	g_pbOut = "{}";
	g_calls.clear();
	g_boostContexts.clear();
	g_run = 0;
	g_hostLoopRules = (eHostLoopRules)rules;
	std::shared_ptr<LoadedModel> lm = std::make_shared<LoadedModel>();
	HRESULT hr = loadVocabulary( modelPath, lm->vocab );
	if( FAILED( hr ) ) return hr;
	{
		void* w = ref_init( modelPath );
		if( !w ) return E_FAIL;
		int32_t h[ 11 ];
		ref_hparams( w, h );
		ref_free( w );
		lm->hp = wh_hparams{ h[ 0 ], h[ 1 ], h[ 2 ], h[ 3 ], h[ 4 ], h[ 5 ], h[ 6 ], h[ 7 ], h[ 8 ], h[ 9 ], h[ 10 ] };
	}
	lm->gpu = fake_model_create( modelPath, threads );
	TestModel model( lm );
	std::vector<MemoryBuffer> buffers( (size_t)nBuffers );
	for( int b = 0; b < nBuffers; b++ ) buffers[ b ].pcm.assign( pcm[ b ], pcm[ b ] + nSamples[ b ] );
	std::vector<sBatchStream> descs( (size_t)nStreams );
	for( int i = 0; i < nStreams; i++ )
		descs[ i ] = sBatchStream{ streams[ i ].buffer >= 0 ? &buffers[ streams[ i ].buffer ] : nullptr, streams[ i ].firstSample, streams[ i ].countSamples, nullptr };
	sFullParams p{};
	p.strategy = eSamplingStrategy::Greedy;
	p.cpuThreads = threads;
	p.n_max_text_ctx = nMaxTextCtx >= 0 ? nMaxTextCtx : 16384;
	p.flags = (eFullParamsFlags)flags;
	p.language = language;
	p.thold_pt = p.thold_ptsum = 0.01f;
	p.prompt_tokens = promptTokens; p.prompt_n_tokens = nPrompt;
	const sBatchSetup setup{ maxSlots, groups, chunk, lookahead };
	iBatchRunner* runner = nullptr;
	hr = createBatchRunner( &model, &setup, &runner );
	if( FAILED( hr ) ) return hr;
	std::ostringstream o;
	for( g_run = 0; g_run < nRuns; g_run++ )
	{
		const int step = script[ g_run ];
		if( step == 1 || step == 2 || step == 3 ) hr = setA( runner );
		if( SUCCEEDED( hr ) && step == 3 ) hr = setA( runner );
		if( SUCCEEDED( hr ) && step == 4 ) hr = setB( runner );
		if( SUCCEEDED( hr ) && ( step == 0 || step == 2 ) ) hr = setBatchBoostedPhrases( runner, nullptr );
		if( SUCCEEDED( hr ) && step == 5 )
		{
			const sBoostedPhrases none{ nullptr, nullptr, 0, 0, 0.0f };
			hr = setBatchBoostedPhrases( runner, &none );
		}
		if( SUCCEEDED( hr ) && step == 6 )
		{
			const int32_t token = lm->vocab.token_eot, len = 1;
			const sBoostedPhrases bad{ &token, &len, 1, 1, 1.0f };
			hr = setBatchBoostedPhrases( runner, &bad );
		}
		if( FAILED( hr ) )
		{
			runner->Release();
			return hr;
		}
		std::vector<iTranscribeResult*> results( (size_t)nStreams, nullptr );
		std::vector<HRESULT> per( (size_t)nStreams, S_OK );
		hr = runner->run( p, descs.data(), (uint32_t)nStreams, results.data(), per.data() );
		o.str( "" );
		o << "{\"hr\":" << hr << ",\"streams\":[";
		for( int i = 0; i < nStreams; i++ )
		{
			o << ( i ? "," : "" ) << "{\"hr\":" << per[ i ] << ",\"segments\":[";
			if( results[ i ] )
			{
				sTranscribeLength len{};
				results[ i ]->getSize( len );
				const sSegment* segs = results[ i ]->getSegments();
				const sToken* toks = results[ i ]->getTokens();
				for( uint32_t s = 0; s < len.countSegments; s++ )
				{
					o << ( s ? "," : "" ) << "{\"t0\":" << segs[ s ].time.begin.ticks << ",\"t1\":" << segs[ s ].time.end.ticks << ",\"text\":";
					jsonString( o, segs[ s ].text );
					o << ",\"tokens\":[";
					for( uint32_t j = 0; j < segs[ s ].countTokens; j++ ) o << ( j ? "," : "" ) << toks[ segs[ s ].firstToken + j ].id;
					o << "]}";
				}
				results[ i ]->Release();
			}
			o << "]}";
		}
		o << "]";
	}
	o << ",\"calls\":[";
	for( size_t k = 0; k < g_calls.size(); k++ )
	{
		const BoostCall& c = g_calls[ k ];
		o << ( k ? "," : "" ) << "{\"context\":" << c.context << ",\"run\":" << c.run << ",\"starts\":" << c.starts << ",\"count\":" << c.count << ",\"first\":" << c.first
		  << ",\"boost\":" << c.boost << "}";
	}
	// fake_device_counters sums over the contexts alive: read before the runner gives its own back
	int64_t counters[ 6 ];
	fake_device_counters( counters );
	o << "],\"counters\":[";
	for( int i = 0; i < 6; i++ ) o << ( i ? "," : "" ) << counters[ i ];
	o << "]}";
	g_pbOut = o.str();
	runner->Release();
	return hr;
}
extern "C" __attribute__( ( visibility( "default" ) ) ) const char* pb_result() { return g_pbOut.c_str(); }
