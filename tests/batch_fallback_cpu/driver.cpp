// tests/batch_fallback_cpu/driver.cpp -- CPU test harness for the decoding fallback of the lock-step batch scheduler (not part of the product).
// One translation unit = the test double of the compute layer (tests/hostloop_cpu/fake_device.cpp) and the batch harness (batch_driver.cpp), both UNCHANGED,
// next to whisper_amd/host/batchScheduler.cpp, plus
//   * the sampling hooks the scheduler gets injected (batchSampling.h g_batchSamplingHooks): they RECORD every ( context, slot, temperature, seed, nonce ) of
//     every round and answer a scripted no-speech probability per stream and window. The double decodes greedily whatever the temperature, so a retried
//     window reproduces its tokens: what is under test is the scheduler -- who keeps which slot, what is uploaded, what becomes of a window;
//   * bf_run: bt_run with the fallback's parameters, an offset, and the per-stream window statistics in its output.
// With -DBF_STANDALONE the file has a main of its own (model path, raw FP32 PCM path): the scenarios of tests/test_batch_fallback_cpu.py once more, for a build
// under -fsanitize=address,undefined.
#include "../hostloop_cpu/fake_device.cpp"
#include "../hostloop_cpu/batch_driver.cpp"
#include "batchSampling.h"
#include <map>

namespace Whisper
{
	HRESULT setBatchDecodingFallback( iBatchRunner* runner, const sDecodingFallback* params );	   // batchScheduler.cpp
	HRESULT getResultWindowStats( const iTranscribeResult* result, sWindowStats* stats, uint32_t* count );
}

namespace
{
	constexpr uint64_t IDLE_SEED = 0;	  // the scheduler gives an idle slot seed 0: the tests use a base seed above the number of streams
	struct RowRecord
	{
		int32_t round, context, slot;
		float temperature;
		uint64_t seed;
		uint32_t nonce;
		int32_t gather;	   // the no-speech switch the scheduler set for this round (filled in by setNoSpeech)
	};
	std::vector<RowRecord> g_rows;
	std::map<wh_context*, int> g_contextIds;
	std::map<wh_context*, std::vector<RowRecord>> g_lastRound;	 // per context: the rows of its round in progress
	int g_rounds = 0, g_reads = 0, g_offCalls = 0;
	uint64_t g_baseSeed = 0;
	int g_failSetAtRound = -1;	   // the round whose upload fails (a device error in the middle of a run)
	// no-speech script: value of stream i's k-th window (the k-th greedy attempt the stream has read); beyond the list: g_noSpeechDefault
	std::map<int, std::vector<float>> g_script;
	std::map<int, int> g_windowOrdinal;
	float g_noSpeechDefault = 0.0f;

	int hookSetRows( wh_context* c, int rows, const float* temperature, const uint64_t* seed, const uint32_t* nonce )
	{
		if( !c ) return WH_E_INVALIDARG;
		if( rows == 0 ) { g_offCalls++; return 0; }
		if( !temperature || !seed || !nonce || rows != c->batch ) return WH_E_INVALIDARG;	   // behind wh_encode_windows of the same round
		if( g_rounds == g_failSetAtRound ) { g_rounds++; return -1; }
		if( !g_contextIds.count( c ) ) { const int id = (int)g_contextIds.size(); g_contextIds[ c ] = id; }
		std::vector<RowRecord>& last = g_lastRound[ c ];
		last.clear();
		for( int b = 0; b < rows; b++ ) last.push_back( RowRecord{ g_rounds, g_contextIds[ c ], b, temperature[ b ], seed[ b ], nonce[ b ], -1 } );
		g_rounds++;
		return 0;
	}
	int hookSetNoSpeech( wh_context* c, int on )
	{
		if( !c ) return WH_E_INVALIDARG;
		auto it = g_lastRound.find( c );
		if( it == g_lastRound.end() ) return 0;	   // the switch-off of a run without the feature
		for( RowRecord& r : it->second ) r.gather = on;
		g_rows.insert( g_rows.end(), it->second.begin(), it->second.end() );
		return 0;
	}
	int hookReadNoSpeech( wh_context* c, float* out )
	{
		auto it = g_lastRound.find( c );
		if( !c || !out || it == g_lastRound.end() || it->second.empty() || !it->second[ 0 ].gather ) return WH_E_INVALIDARG;	  // read without a gather
		g_reads++;
		for( const RowRecord& r : it->second )
		{
			out[ r.slot ] = -1.0f;		  // an idle slot, or a retrying one: the scheduler must not use it
			if( r.seed == IDLE_SEED || ( r.nonce & 7u ) != 0 ) continue;
			const int stream = (int)( r.seed - g_baseSeed );
			const int k = g_windowOrdinal[ stream ]++;
			const std::vector<float>& v = g_script[ stream ];
			out[ r.slot ] = k < (int)v.size() ? v[ (size_t)k ] : g_noSpeechDefault;
		}
		return 0;
	}
	const Whisper::BatchSamplingHooks g_hooks = { &hookSetRows, &hookSetNoSpeech, &hookReadNoSpeech };
	std::string g_fbOut;
}

extern "C" __attribute__( ( visibility( "default" ) ) ) void bf_install_hooks( int install ) { Whisper::g_batchSamplingHooks = install ? &g_hooks : nullptr; }
// stream's windows get these no-speech probabilities in order (n == 0 clears every script); later windows get `dflt`
extern "C" __attribute__( ( visibility( "default" ) ) ) void bf_script_no_speech( int stream, const float* values, int n, float dflt )
{
	if( n == 0 ) g_script.clear();
	else g_script[ stream ].assign( values, values + n );
	g_noSpeechDefault = dflt;
}
extern "C" __attribute__( ( visibility( "default" ) ) ) void bf_fail_upload_at_round( int round ) { g_failSetAtRound = round; }
// the records of the last bf_run: *count rows; out may be NULL
extern "C" __attribute__( ( visibility( "default" ) ) ) void bf_rows( RowRecord* out, int cap, int* count, int* reads, int* offCalls )
{
	*count = (int)g_rows.size();
	if( reads ) *reads = g_reads;
	if( offCalls ) *offCalls = g_offCalls;
	if( out )
		for( int i = 0; i < cap && i < (int)g_rows.size(); i++ ) out[ i ] = g_rows[ (size_t)i ];
}

// bt_run's arguments, then: fallbackOn (0 = never set, 1 = set, 2 = set and turned off again with nullptr before the run), the sDecodingFallback fields, offsetMs.
// Returns the run's HRESULT, or the HRESULT of setBatchDecodingFallback when that fails (bf_result() then is "{}").
// bf_result() = bt_result's streams with "stats":[{"seek","attempts","temperature","no_speech","avg_logprob","entropy","skipped"}] each, and "counters":
// fake_device_counters at the end of the run, while the runner's contexts are alive.
extern "C" __attribute__( ( visibility( "default" ) ) ) int bf_run( const char* modelPath, int rules, uint32_t flags, uint32_t language, int nMaxTextCtx,
	const int32_t* promptTokens, int nPrompt, const float* const* pcm, const int32_t* nSamples, int nBuffers, const BatchStreamDesc* streams, int nStreams,
	uint32_t maxSlots, uint32_t groups, uint32_t chunk, uint32_t lookahead, int threads, int fallbackOn, float temperatureInc, float logprobThold,
	float entropyThold, float noSpeechThold, uint64_t seed, int offsetMs )
{
	g_fbOut = "{}";
	g_rows.clear();
	g_lastRound.clear();
	g_contextIds.clear();
	g_windowOrdinal.clear();
	g_rounds = g_reads = g_offCalls = 0;
	g_baseSeed = seed;
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
	p.offset_ms = offsetMs;
	const sBatchSetup setup{ maxSlots, groups, chunk, lookahead };
	iBatchRunner* runner = nullptr;
	hr = createBatchRunner( &model, &setup, &runner );
	if( FAILED( hr ) ) return hr;
	if( fallbackOn )
	{
		sDecodingFallback f;
		f.temperatureInc = temperatureInc; f.logprobThold = logprobThold; f.entropyThold = entropyThold; f.noSpeechThold = noSpeechThold; f.seed = seed;
		hr = setBatchDecodingFallback( runner, &f );
		if( SUCCEEDED( hr ) && fallbackOn == 2 ) hr = setBatchDecodingFallback( runner, nullptr );
		if( FAILED( hr ) )
		{
			runner->Release();
			return hr;
		}
	}
	std::vector<iTranscribeResult*> results( (size_t)nStreams, nullptr );
	std::vector<HRESULT> per( (size_t)nStreams, S_OK );
	hr = runner->run( p, descs.data(), (uint32_t)nStreams, results.data(), per.data() );
	std::ostringstream o;
	o.precision( 17 );
	o << "{\"hr\":" << hr << ",\"streams\":[";
	for( int i = 0; i < nStreams; i++ )
	{
		o << ( i ? "," : "" ) << "{\"hr\":" << per[ i ] << ",\"segments\":[";
		std::vector<sWindowStats> stats;
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
			uint32_t n = 0;
			if( SUCCEEDED( getResultWindowStats( results[ i ], nullptr, &n ) ) && n > 0 )
			{
				stats.resize( n );
				if( FAILED( getResultWindowStats( results[ i ], stats.data(), &n ) ) ) stats.clear();
			}
			results[ i ]->Release();
		}
		o << "],\"stats\":[";
		for( size_t k = 0; k < stats.size(); k++ )
		{
			const sWindowStats& w = stats[ k ];
			o << ( k ? "," : "" ) << "{\"seek\":" << w.seek << ",\"attempts\":" << w.attempts << ",\"temperature\":" << (double)w.temperature << ",\"no_speech\":"
			  << (double)w.noSpeech << ",\"avg_logprob\":" << w.avgLogprob << ",\"entropy\":" << w.entropy << ",\"skipped\":" << w.skipped << "}";
		}
		o << "]}";
	}
	// fake_device_counters sums over the contexts alive: read before the runner gives its own back
	int64_t counters[ 6 ];
	fake_device_counters( counters );
	o << "],\"counters\":[";
	for( int i = 0; i < 6; i++ ) o << ( i ? "," : "" ) << counters[ i ];
	o << "]}";
	g_fbOut = o.str();
	runner->Release();
	return hr;
}
extern "C" __attribute__( ( visibility( "default" ) ) ) const char* bf_result() { return g_fbOut.c_str(); }

#ifdef BF_STANDALONE
// The scenarios once more in a program of its own: every gate failing (six attempts per window) at 1, 2 and 5 slots, a silent window under carry-over, the
// feature off, and an upload that fails while streams retry. Prints one line per scenario; exit status 0 when every run answered what it should.
#include <fstream>
int main( int argc, char** argv )
{
	if( argc < 3 ) { fprintf( stderr, "usage: %s model.bin pcm.f32\n", argv[ 0 ] ); return 2; }
	std::ifstream f( argv[ 2 ], std::ios::binary );
	std::vector<char> raw( ( std::istreambuf_iterator<char>( f ) ), std::istreambuf_iterator<char>() );
	std::vector<float> all( raw.size() / 4 );
	memcpy( all.data(), raw.data(), all.size() * 4 );
	if( all.size() < 16000 * 8 ) { fprintf( stderr, "the PCM file is too short\n" ); return 2; }
	std::vector<float> half( all.begin(), all.begin() + (ptrdiff_t)( all.size() / 2 ) );
	const float* pcm[ 2 ] = { all.data(), half.data() };
	const int32_t lens[ 2 ] = { (int32_t)all.size(), (int32_t)half.size() };
	const BatchStreamDesc streams[ 4 ] = { { 0, 0, 0 }, { 1, 0, 0 }, { 0, 16000 * 2, 16000 * 5 }, { 1, 0, 0 } };
	const int32_t prompt[ 1 ] = { 1000 };
	const uint32_t en = 0x6e65u;	// "en"
	const float inf = 1e30f;
	int bad = 0;
	bf_install_hooks( 1 );
	for( uint32_t slots : { 1u, 2u, 5u } )
	{
		const int hr = bf_run( argv[ 1 ], 0, 0, en, 16, prompt, 1, pcm, lens, 2, streams, 4, slots, 1, 4, 0, 2, 1, 0.2f, inf, -1.0f, 2.0f, 1000, 0 );
		printf( "always-fail, %u slots: hr 0x%08x, %d row records\n", slots, (unsigned)hr, (int)g_rows.size() );
		bad += hr != 0 || g_rows.empty();
	}
	{
		const float silent[ 1 ] = { 0.9f };
		bf_script_no_speech( 1, silent, 1, 0.0f );
		const int hr = bf_run( argv[ 1 ], 0, 0, en, 16, prompt, 1, pcm, lens, 2, streams, 4, 2, 2, 3, 1, 2, 1, 0.0f, inf, -1.0f, 0.5f, 1000, 0 );
		printf( "a silent window: hr 0x%08x\n", (unsigned)hr );
		bad += hr != 0;
		bf_script_no_speech( 0, nullptr, 0, 0.0f );
	}
	{
		const int hr = bf_run( argv[ 1 ], 0, 0, en, 16, prompt, 1, pcm, lens, 2, streams, 4, 2, 1, 4, 0, 2, 2, 0.2f, inf, -1.0f, 2.0f, 1000, 0 );
		printf( "feature off: hr 0x%08x, %d row records\n", (unsigned)hr, (int)g_rows.size() );
		bad += hr != 0 || !g_rows.empty();
	}
	{
		bf_fail_upload_at_round( 3 );
		const int hr = bf_run( argv[ 1 ], 0, 0, en, 16, prompt, 1, pcm, lens, 2, streams, 4, 2, 1, 4, 0, 2, 1, 0.2f, inf, -1.0f, 2.0f, 1000, 0 );
		bf_fail_upload_at_round( -1 );
		printf( "upload fails in round 3: hr 0x%08x\n", (unsigned)hr );
		bad += hr >= 0;
	}
	bf_install_hooks( 0 );
	{
		const int hr = bf_run( argv[ 1 ], 0, 0, en, 16, prompt, 1, pcm, lens, 2, streams, 4, 2, 1, 4, 0, 2, 1, 0.2f, inf, -1.0f, 2.0f, 1000, 0 );
		printf( "no hooks: hr 0x%08x\n", (unsigned)hr );
		bad += (unsigned)hr != 0x80004001u;
	}
	printf( bad ? "FAILED\n" : "standalone ok\n" );
	return bad ? 1 : 0;
}
#endif
