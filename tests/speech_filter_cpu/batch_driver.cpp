// tests/speech_filter_cpu/batch_driver.cpp -- CPU test harness for the speech filter in the lock-step batch scheduler (not part of the product).
// One translation unit = the test double of the compute layer (tests/hostloop_cpu/fake_device.cpp) and the batch harness (batch_driver.cpp), both UNCHANGED,
// next to whisper_amd/host/batchScheduler.cpp, plus
//   * the packer the scheduler gets injected (batchSpeech.h g_batchSpeechPacker): a HOST copy. The double's device buffers are host memory, so the packer reads
//     the stream's samples where the scheduler uploaded them, calls a frame speech when one of its samples is larger than SF_THRESHOLD in magnitude (the real
//     detector needs the device), applies the span rules of speechSpans.h and copies the spans into a buffer of its own -- one per call, all kept until the run
//     is over, so that a spectrogram taken later would still read the right samples;
//   * sf_run: bt_run with Whisper::setBatchSpeechFilter applied first. mode 0: no call; 1: set( params ); 2: set( params ), then set( nullptr ).
// sf_result() = bt_result's streams, each with "spans":[[a,b]] (getResultSpeechSpans), and "packer_calls".
#include "../hostloop_cpu/fake_device.cpp"
#include "../hostloop_cpu/batch_driver.cpp"
#include "batchSpeech.h"
#include "speechSpans.h"
#include <cmath>
#include <list>

namespace Whisper
{
	HRESULT setBatchSpeechFilter( iBatchRunner* runner, const sSpeechFilter* params );	 // batchScheduler.cpp
	HRESULT getResultSpeechSpans( const iTranscribeResult* result, sSpeechSpan* spans, uint32_t* count );
}

namespace
{
	constexpr float SF_THRESHOLD = 0.005f;
	std::list<std::vector<float>> g_packed;
	int g_packerCalls = 0;
	std::string g_sfOut;

	int hostPacker( wh_context* c, const float* pcmDev, int64_t nSamples, const float* stereoDev, const wh_speech_params* params, const float** packedDev,
		const float** packedStereoDev, int64_t* nPacked, int64_t* spansOut, int cap, int* count )
	{
		if( !c || !packedDev || !nPacked || !count || nSamples < 0 || stereoDev ) return WH_E_INVALIDARG;
		g_packerCalls++;
		const int64_t nFrames = nSamples / 256;
		std::vector<uint8_t> speech( (size_t)nFrames, 0 );
		for( int64_t f = 0; f < nFrames; f++ )
			for( int k = 0; k < 256 && !speech[ (size_t)f ]; k++ )
				if( std::fabs( pcmDev[ f * 256 + k ] ) > SF_THRESHOLD ) speech[ (size_t)f ] = 1;
		std::vector<speechRules::Span> spans;
		if( FAILED( speechRules::find( speech.data(), nFrames, nSamples, params ? params->minSilenceFrames : 0, params ? params->minSpeechFrames : 0,
				params ? params->padFrames : 0, spans ) ) )
			return WH_E_INVALIDARG;
		*count = (int)spans.size();
		*packedDev = nullptr;
		if( packedStereoDev ) *packedStereoDev = nullptr;
		*nPacked = speechRules::packedLength( spans );
		if( (int)spans.size() > cap ) return WH_E_BOUNDS;
		for( size_t i = 0; i < spans.size(); i++ ) { spansOut[ 2 * i ] = spans[ i ].a; spansOut[ 2 * i + 1 ] = spans[ i ].b; }
		if( spans.empty() ) return 0;
		if( speechRules::coversAll( spans, nSamples ) ) { *packedDev = pcmDev; return 0; }
		g_packed.emplace_back();
		std::vector<float>& out = g_packed.back();
		for( const speechRules::Span& s : spans ) out.insert( out.end(), pcmDev + s.a, pcmDev + s.b );
		*packedDev = out.data();
		return 0;
	}
}

extern "C" __attribute__( ( visibility( "default" ) ) ) void sf_install_hook( int install ) { Whisper::g_batchSpeechPacker = install ? &hostPacker : nullptr; }

extern "C" __attribute__( ( visibility( "default" ) ) ) int sf_run( const char* modelPath, int rules, uint32_t flags, uint32_t language, int nMaxTextCtx,
	const int32_t* promptTokens, int nPrompt, const float* const* pcm, const int32_t* nSamples, int nBuffers, const BatchStreamDesc* streams, int nStreams,
	uint32_t maxSlots, uint32_t groups, uint32_t chunk, uint32_t lookahead, int threads, int mode, int minSilence, int minSpeech, int pad )
{
	g_sfOut = "{}";
	g_packed.clear();
	g_packerCalls = 0;
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
	const sSpeechFilter filter{ minSilence, minSpeech, pad, 0 };
	if( mode >= 1 ) hr = setBatchSpeechFilter( runner, &filter );
	if( SUCCEEDED( hr ) && mode == 2 ) hr = setBatchSpeechFilter( runner, nullptr );
	if( FAILED( hr ) )
	{
		runner->Release();
		return hr;
	}
	std::vector<iTranscribeResult*> results( (size_t)nStreams, nullptr );
	std::vector<HRESULT> per( (size_t)nStreams, S_OK );
	hr = runner->run( p, descs.data(), (uint32_t)nStreams, results.data(), per.data() );
	std::ostringstream o;
	o << "{\"hr\":" << hr << ",\"streams\":[";
	for( int i = 0; i < nStreams; i++ )
	{
		o << ( i ? "," : "" ) << "{\"hr\":" << per[ i ] << ",\"result\":" << ( results[ i ] ? 1 : 0 ) << ",\"segments\":[";
		std::vector<sSpeechSpan> spans;
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
			if( SUCCEEDED( getResultSpeechSpans( results[ i ], nullptr, &n ) ) && n > 0 )
			{
				spans.resize( n );
				getResultSpeechSpans( results[ i ], spans.data(), &n );
			}
			results[ i ]->Release();
		}
		o << "],\"spans\":[";
		for( size_t k = 0; k < spans.size(); k++ ) o << ( k ? "," : "" ) << "[" << spans[ k ].firstSample << "," << spans[ k ].endSample << "]";
		o << "]}";
	}
	o << "],\"packer_calls\":" << g_packerCalls << "}";
	g_sfOut = o.str();
	runner->Release();
	g_packed.clear();
	return hr;
}
extern "C" __attribute__( ( visibility( "default" ) ) ) const char* sf_result() { return g_sfOut.c_str(); }
