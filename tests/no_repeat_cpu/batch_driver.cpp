// tests/no_repeat_cpu/batch_driver.cpp -- CPU test harness for no-repeat n-grams in the lock-step batch scheduler (not part of the product).
// One translation unit = the test double of the compute layer (tests/hostloop_cpu/fake_device.cpp) and the batch harness (batch_driver.cpp), both UNCHANGED,
// next to whisper_amd/host/batchScheduler.cpp, plus
//   * the hook the scheduler gets injected (batchNoRepeat.h g_batchNoRepeat): it RECORDS every call -- which context, in which run, how many window starts that
//     context had seen, which n -- and filters nothing (the double has no logits to filter), so the transcripts must be those of a runner on which nothing was set;
//   * nr_run: bt_run with a script of calls, one entry applied before each of the runs of ONE runner.
#include "../hostloop_cpu/fake_device.cpp"
#include "../hostloop_cpu/batch_driver.cpp"
#include "batchNoRepeat.h"
#include <map>

namespace Whisper
{
	HRESULT setBatchNoRepeatNgram( iBatchRunner* runner, int n );	 // batchScheduler.cpp
}

namespace
{
	struct RulesCall { int context, run, starts, n; };
	std::vector<RulesCall> g_calls;
	std::map<wh_context*, int> g_rulesContexts;
	int g_run = 0;
	std::string g_trOut;

	int hookRules( wh_context* c, int n )
	{
		if( !c ) return WH_E_INVALIDARG;
		if( !g_rulesContexts.count( c ) ) { const int id = (int)g_rulesContexts.size(); g_rulesContexts[ c ] = id; }
		g_calls.push_back( RulesCall{ g_rulesContexts[ c ], g_run, c->starts, n } );
		return 0;
	}
}

extern "C" __attribute__( ( visibility( "default" ) ) ) void nr_install_hook( int install ) { Whisper::g_batchNoRepeat = install ? &hookRules : nullptr; }

// bt_run's arguments, then a script: before run r (r = 0 .. nRuns - 1) script[ r ] is applied: -100 = no call, 100 + k = setBatchNoRepeatNgram( k ) and then
// ( 0 ), any other value x = setBatchNoRepeatNgram( x ), whatever x is. Returns the last run's HRESULT, or the HRESULT of setBatchNoRepeatNgram when that fails
// (nr_result() then is "{}").
// nr_result() = bt_result's streams of the last run, "calls":[{"context","run","starts","n"}] and "counters": fake_device_counters while the runner is alive.
extern "C" __attribute__( ( visibility( "default" ) ) ) int nr_run( const char* modelPath, int rules, uint32_t flags, uint32_t language, int nMaxTextCtx,
	const int32_t* promptTokens, int nPrompt, const float* const* pcm, const int32_t* nSamples, int nBuffers, const BatchStreamDesc* streams, int nStreams,
	uint32_t maxSlots, uint32_t groups, uint32_t chunk, uint32_t lookahead, int threads, const int32_t* script, int nRuns )
{
	g_trOut = "{}";
	g_calls.clear();
	g_rulesContexts.clear();
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
		if( step >= 100 )
		{
			hr = setBatchNoRepeatNgram( runner, step - 100 );
			if( SUCCEEDED( hr ) ) hr = setBatchNoRepeatNgram( runner, 0 );
		}
		else if( step != -100 ) hr = setBatchNoRepeatNgram( runner, step );
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
		const RulesCall& c = g_calls[ k ];
		o << ( k ? "," : "" ) << "{\"context\":" << c.context << ",\"run\":" << c.run << ",\"starts\":" << c.starts << ",\"n\":" << c.n << "}";
	}
	// fake_device_counters sums over the contexts alive: read before the runner gives its own back
	int64_t counters[ 6 ];
	fake_device_counters( counters );
	o << "],\"counters\":[";
	for( int i = 0; i < 6; i++ ) o << ( i ? "," : "" ) << counters[ i ];
	o << "]}";
	g_trOut = o.str();
	runner->Release();
	return hr;
}
extern "C" __attribute__( ( visibility( "default" ) ) ) const char* nr_result() { return g_trOut.c_str(); }
