// tests/suppress_cpu/batch_driver.cpp -- CPU test harness for suppressed tokens in the lock-step batch scheduler (not part of the product).
// One translation unit = the test double of the compute layer (tests/hostloop_cpu/fake_device.cpp) and the batch harness (batch_driver.cpp), both UNCHANGED,
// next to whisper_amd/host/batchScheduler.cpp, plus
//   * the hook the scheduler gets injected (batchSuppress.h g_batchSuppress): it RECORDS every call -- which context, how many window starts that context had
//     seen, the ids -- and filters nothing (the double has no logits to filter), so the transcripts must be those of a runner on which nothing was set;
//   * bs_run: bt_run with a set, applied before the first of `nRuns` runs of ONE runner.
#include "../hostloop_cpu/fake_device.cpp"
#include "../hostloop_cpu/batch_driver.cpp"
#include "batchSuppress.h"
#include <map>

namespace Whisper
{
	HRESULT setBatchSuppressedTokens( iBatchRunner* runner, const int32_t* ids, uint32_t count );	   // batchScheduler.cpp
}

namespace
{
	struct SuppressCall
	{
		int context, run, starts;
		std::vector<int32_t> ids;
	};
	std::vector<SuppressCall> g_calls;
	std::map<wh_context*, int> g_suppressContexts;
	int g_run = 0;
	std::string g_bsOut;

	int hookSuppress( wh_context* c, const int32_t* ids, int count )
	{
		if( !c || count < 0 || ( count > 0 && !ids ) ) return WH_E_INVALIDARG;
		if( !g_suppressContexts.count( c ) ) { const int id = (int)g_suppressContexts.size(); g_suppressContexts[ c ] = id; }
		g_calls.push_back( SuppressCall{ g_suppressContexts[ c ], g_run, c->starts, std::vector<int32_t>( ids, ids + count ) } );
		return 0;
	}
}

extern "C" __attribute__( ( visibility( "default" ) ) ) void bs_install_hook( int install ) { Whisper::g_batchSuppress = install ? &hookSuppress : nullptr; }

// bt_run's arguments, then: mode (0 = never set, 1 = the set, 2 = the set and then an empty one before the first run, 3 = an empty set only), the ids, and the
// number of runs of the one runner. Returns the last run's HRESULT, or the HRESULT of setBatchSuppressedTokens when that fails (bs_result() then is "{}").
// bs_result() = bt_result's streams of the last run, "calls":[{"context","run","starts","ids"}] and "counters": fake_device_counters while the runner is alive.
extern "C" __attribute__( ( visibility( "default" ) ) ) int bs_run( const char* modelPath, int rules, uint32_t flags, uint32_t language, int nMaxTextCtx,
	const int32_t* promptTokens, int nPrompt, const float* const* pcm, const int32_t* nSamples, int nBuffers, const BatchStreamDesc* streams, int nStreams,
	uint32_t maxSlots, uint32_t groups, uint32_t chunk, uint32_t lookahead, int threads, int mode, const int32_t* ids, uint32_t nIds, int nRuns )
{
	g_bsOut = "{}";
	g_calls.clear();
	g_suppressContexts.clear();
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
	if( mode == 1 || mode == 2 ) hr = setBatchSuppressedTokens( runner, ids, nIds );
	if( SUCCEEDED( hr ) && ( mode == 2 || mode == 3 ) ) hr = setBatchSuppressedTokens( runner, nullptr, 0 );
	if( FAILED( hr ) )
	{
		runner->Release();
		return hr;
	}
	std::ostringstream o;
	for( g_run = 0; g_run < nRuns; g_run++ )
	{
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
		const SuppressCall& c = g_calls[ k ];
		o << ( k ? "," : "" ) << "{\"context\":" << c.context << ",\"run\":" << c.run << ",\"starts\":" << c.starts << ",\"ids\":[";
		for( size_t j = 0; j < c.ids.size(); j++ ) o << ( j ? "," : "" ) << c.ids[ j ];
		o << "]}";
	}
	// fake_device_counters sums over the contexts alive: read before the runner gives its own back
	int64_t counters[ 6 ];
	fake_device_counters( counters );
	o << "],\"counters\":[";
	for( int i = 0; i < 6; i++ ) o << ( i ? "," : "" ) << counters[ i ];
	o << "]}";
	g_bsOut = o.str();
	runner->Release();
	return hr;
}
extern "C" __attribute__( ( visibility( "default" ) ) ) const char* bs_result() { return g_bsOut.c_str(); }

// Whisper::getNonSpeechTokens on the vocabulary of a model file (no device): out may be NULL, *count in = capacity, out = size
extern "C" __attribute__( ( visibility( "default" ) ) ) int bs_non_speech( const char* modelPath, int32_t* out, uint32_t* count )
{
	std::shared_ptr<LoadedModel> lm = std::make_shared<LoadedModel>();
	const HRESULT hr = loadVocabulary( modelPath, lm->vocab );
	if( FAILED( hr ) ) return hr;
	TestModel model( lm );
	return getNonSpeechTokens( &model, out, count );
}
// Whisper::setBatchSuppressedTokens on a fresh runner over the vocabulary of a model file: the argument checks alone
extern "C" __attribute__( ( visibility( "default" ) ) ) int bs_set_only( const char* modelPath, const int32_t* ids, uint32_t count )
{
	std::shared_ptr<LoadedModel> lm = std::make_shared<LoadedModel>();
	HRESULT hr = loadVocabulary( modelPath, lm->vocab );
	if( FAILED( hr ) ) return hr;
	TestModel model( lm );
	const sBatchSetup setup{ 2, 1, 4, 0 };
	iBatchRunner* runner = nullptr;
	hr = createBatchRunner( &model, &setup, &runner );
	if( FAILED( hr ) ) return hr;
	hr = setBatchSuppressedTokens( runner, ids, count );
	runner->Release();
	return hr;
}
