// tests/hostloop_cpu/batch_lang_driver.cpp -- CPU test harness for language "auto" in the lock-step batch scheduler (not part of the product).
// One translation unit = the test double of the compute layer (fake_device.cpp) and the batch harness (batch_driver.cpp), both UNCHANGED, plus
//   * the language detector the scheduler gets injected (languageDetect.h g_batchLanguageDetector): the device half of whisper_lang_auto_detect played by
//     the double's per-slot reference models -- [sot] at position 0 through whisper_decode, the probabilities at the language tokens;
//   * bl_run: bt_run with a per-stream language in its output (what whisperc_tr_language reads from a result).
#include "fake_device.cpp"
#include "batch_driver.cpp"
#include "languageDetect.h"

extern "C" {
size_t ref_logits_size( void* ctx );
void ref_get_probs( void* ctx, float* dst );
}

namespace
{
	int g_detectCalls = 0, g_detectWindows = 0;
	// wh_lang_detect of include/whisper_hip.h over the double: the slots wh_encode_windows marked active are detected, the idle ones report zeros
	int fakeLangDetect( wh_context* c, int batch, float* langP, int32_t* best )
	{
		if( !c || batch != c->batch ) return WH_E_INVALIDARG;
		g_detectCalls++;
		for( int b = 0; b < batch; b++ )
		{
			best[ b ] = 0;
			if( !c->active[ b ] ) continue;
			g_detectWindows++;
			void* w = c->cpu[ b ];
			int32_t hp[ 11 ];
			ref_hparams( w, hp );
			const int nVocab = hp[ 0 ], nLang = nVocab - 51766, sot = 50258;
			const int32_t tok = sot;
			if( 0 != ref_decode( w, &tok, 1, 0, c->model->threads ) ) return -1;
			std::vector<float> probs( ref_logits_size( w ) );
			ref_get_probs( w, probs.data() );
			const float* p = probs.data() + probs.size() - nVocab + sot + 1;
			for( int i = 0; i < nLang; i++ )
			{
				if( langP ) langP[ (size_t)b * nLang + i ] = p[ i ];
				if( p[ i ] > p[ best[ b ] ] ) best[ b ] = i;
			}
		}
		return 0;
	}
	const bool g_installed = ( Whisper::g_batchLanguageDetector = &fakeLangDetect, true );
	std::string g_langOut;
}

// install = 0: the scheduler without a detector (language "auto" must be E_NOTIMPL per stream)
extern "C" __attribute__( ( visibility( "default" ) ) ) void bl_install_detector( int install )
{
	Whisper::g_batchLanguageDetector = install ? &fakeLangDetect : nullptr;
}
extern "C" __attribute__( ( visibility( "default" ) ) ) void bl_detect_counters( int32_t* out2 ) { out2[ 0 ] = g_detectCalls; out2[ 1 ] = g_detectWindows; }

// bt_run's arguments; bl_result() = {"hr":..,"streams":[{"hr":..,"lang":id or -1,"p":..,"segments":[{"t0","t1","tokens":[ids]}]}]}
extern "C" __attribute__( ( visibility( "default" ) ) ) int bl_run( const char* modelPath, int rules, uint32_t flags, uint32_t language, int nMaxTextCtx,
	const int32_t* promptTokens, int nPrompt, const float* const* pcm, const int32_t* nSamples, int nBuffers, const BatchStreamDesc* streams, int nStreams,
	uint32_t maxSlots, uint32_t groups, uint32_t chunk, uint32_t lookahead, int threads )
{
	g_langOut.clear();
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
	std::vector<iTranscribeResult*> results( (size_t)nStreams, nullptr );
	std::vector<HRESULT> per( (size_t)nStreams, S_OK );
	hr = runner->run( p, descs.data(), (uint32_t)nStreams, results.data(), per.data() );
	std::ostringstream o;
	o << "{\"hr\":" << hr << ",\"streams\":[";
	for( int i = 0; i < nStreams; i++ )
	{
		const TranscribeResult* tr = dynamic_cast<const TranscribeResult*>( results[ i ] );
		o << ( i ? "," : "" ) << "{\"hr\":" << per[ i ] << ",\"lang\":" << ( tr ? tr->languageId : -1 ) << ",\"p\":" << ( tr ? tr->languageP : 0.0f ) << ",\"segments\":[";
		if( results[ i ] )
		{
			sTranscribeLength len{};
			results[ i ]->getSize( len );
			const sSegment* segs = results[ i ]->getSegments();
			const sToken* toks = results[ i ]->getTokens();
			for( uint32_t s = 0; s < len.countSegments; s++ )
			{
				o << ( s ? "," : "" ) << "{\"t0\":" << segs[ s ].time.begin.ticks << ",\"t1\":" << segs[ s ].time.end.ticks << ",\"tokens\":[";
				for( uint32_t j = 0; j < segs[ s ].countTokens; j++ ) o << ( j ? "," : "" ) << toks[ segs[ s ].firstToken + j ].id;
				o << "]}";
			}
			results[ i ]->Release();
		}
		o << "]}";
	}
	o << "]}";
	g_langOut = o.str();
	runner->Release();
	return hr;
}
extern "C" __attribute__( ( visibility( "default" ) ) ) const char* bl_result() { return g_langOut.c_str(); }
