// The flat C mirror of the COM-style API for FFI callers (ctypes / cgo / JNI): see include/whisper_c.h. Every whisperc_* export of libWhisper.so that is not
// scoreTranscripts.cpp's or splitAtPauses.cpp's. Nothing here decides anything: an export turns its plain arguments into the objects of whisperApi.h, calls
// the interface or the function of the same name, and copies the answer out. What the entry points share is stated once, in the namespace below.
#include "hostCommon.h"
#include "hostLoop.h"
#include "languageDetect.h"
#include "results.h"
#include "wavFormat.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>

using namespace Whisper;

namespace
{
	// sFullParams of a whisperc_run_* / whisperc_batch_run* call: the strategy's defaults, then what every one of them takes. An entry point sets only its
	// own fields on top (the range, audio_ctx, the thresholds, the beam width).
	HRESULT fullParams( eSamplingStrategy strategy, const char* language, uint32_t flags, int maxTokens, const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, sFullParams& p )
	{
		CHECK( defaultFullParams( strategy, &p ) );
		p.flags = (eFullParamsFlags)flags;
		p.language = makeLanguageKey( language ? language : "en" );
		p.max_tokens = maxTokens;
		p.prompt_tokens = promptTokens;
		p.prompt_n_tokens = nPrompt;
		if( nMaxTextCtx >= 0 ) p.n_max_text_ctx = nMaxTextCtx;
		return S_OK;
	}
	// interleaved stereo frames of a caller as the vector a buffer or reader takes; NULL: none
	std::vector<float> stereoCopy( const float* stereo, uint32_t nSamples )
	{
		return stereo ? std::vector<float>( stereo, stereo + 2 * (size_t)nSamples ) : std::vector<float>();
	}
	// iContext::runFull over a copy of the caller's PCM
	HRESULT runFullOn( void* ctx, const sFullParams& p, const float* pcm, const float* stereo, uint32_t nSamples )
	{
		iAudioBuffer* buf = nullptr;
		CHECK( createAudioBuffer( std::vector<float>( pcm, pcm + nSamples ), stereoCopy( stereo, nSamples ), &buf ) );
		const HRESULT hr = ( (iContext*)ctx )->runFull( p, buf );
		buf->Release();
		return hr;
	}
	// iContext::runStreamed over a reader, which is released: progress values are appended to progressOut (up to progressCap), their count is returned
	// through progressCount
	HRESULT runStreamedOn( void* ctx, const sFullParams& p, iAudioReader* reader, double* progressOut, int progressCap, int* progressCount )
	{
		struct Sink { double* out; int cap, n; } sink{ progressOut, progressCap, 0 };
		sProgressSink ps;
		ps.pfn = []( double v, iContext*, void* pv ) noexcept -> HRESULT
		{
			Sink* s = (Sink*)pv;
			if( s->out && s->n < s->cap ) s->out[ s->n ] = v;
			s->n++;
			return S_OK;
		};
		ps.pv = &sink;
		const HRESULT hr = ( (iContext*)ctx )->runStreamed( p, ps, reader );
		reader->Release();
		if( progressCount ) *progressCount = sink.n;
		return hr;
	}

	// What the whisperc_tr_* exports answer for a result; the whisperc_result_* forms ask the same of a context's results
	HRESULT contextResults( void* ctx, iTranscribeResult*& r )
	{
		return ( (iContext*)ctx )->getResults( eResultFlags::Tokens | eResultFlags::Timestamps, &r );
	}
	HRESULT resultCounts( iTranscribeResult* r, uint32_t* segments, uint32_t* tokens )
	{
		if( !r || !segments || !tokens ) return E_POINTER;
		sTranscribeLength len;
		r->getSize( len );
		*segments = len.countSegments;
		*tokens = len.countTokens;
		return S_OK;
	}
	// segment times in 10 ms units are returned as 100 ns ticks like the COM API
	HRESULT resultSegment( iTranscribeResult* r, uint32_t index, uint64_t* t0, uint64_t* t1, uint32_t* firstToken, uint32_t* countTokens, char* text, uint32_t textCap )
	{
		if( !r ) return E_POINTER;
		sTranscribeLength len;
		r->getSize( len );
		if( index >= len.countSegments ) return E_BOUNDS;
		const sSegment& s = r->getSegments()[ index ];
		*t0 = s.time.begin.ticks; *t1 = s.time.end.ticks; *firstToken = s.firstToken; *countTokens = s.countTokens;
		if( text && textCap ) snprintf( text, textCap, "%s", s.text ? s.text : "" );
		return S_OK;
	}
	// the exports copy out the fields they have arguments for
	HRESULT resultToken( iTranscribeResult* r, uint32_t index, const sToken*& t )
	{
		if( !r ) return E_POINTER;
		sTranscribeLength len;
		r->getSize( len );
		if( index >= len.countTokens ) return E_BOUNDS;
		t = r->getTokens() + index;
		return S_OK;
	}

	// whisperc_set_fallback / whisperc_batch_set_fallback: on != 0 turns the feature on with these parameters, 0 turns it off (the others are ignored)
	template<class I>
	HRESULT setFallbackOn( HRESULT ( *set )( I*, const sDecodingFallback* ), void* object, int32_t on, float temperatureInc, float logprobThold, float entropyThold, float noSpeechThold, uint64_t seed )
	{
		if( !object ) return E_POINTER;
		if( !on ) return set( (I*)object, nullptr );
		sDecodingFallback p;
		p.temperatureInc = temperatureInc; p.logprobThold = logprobThold; p.entropyThold = entropyThold; p.noSpeechThold = noSpeechThold; p.seed = seed;
		return set( (I*)object, &p );
	}
}

extern "C" {

WHISPER_EXPORT int32_t whisperc_load_model( const char* pathUtf8, int device, void** modelOut )
{
	if( !pathUtf8 || !modelOut ) return E_POINTER;
	std::wstring w;
	for( const unsigned char* p = (const unsigned char*)pathUtf8; *p; p++ ) w += (wchar_t)*p;	// paths used by the tests are ASCII
	std::wstring adapter = std::to_wstring( device ) + L":";
	sModelSetup setup;
	setup.adapter = adapter.c_str();
	iModel* m = nullptr;
	const HRESULT hr = loadModel( w.c_str(), setup, nullptr, &m );
	*modelOut = m;
	return hr;
}
WHISPER_EXPORT void whisperc_release( void* unknown )
{
	if( unknown ) ( (ComLight::IUnknown*)unknown )->Release();
}
WHISPER_EXPORT int32_t whisperc_create_context( void* model, void** ctxOut )
{
	if( !model || !ctxOut ) return E_POINTER;
	iContext* c = nullptr;
	const HRESULT hr = ( (iModel*)model )->createContext( &c );
	*ctxOut = c;
	return hr;
}
WHISPER_EXPORT int32_t whisperc_special_tokens( void* model, int32_t* out8 )
{
	SpecialTokens st;
	const HRESULT hr = ( (iModel*)model )->getSpecialTokens( st );
	memcpy( out8, &st, sizeof( st ) );
	return hr;
}
WHISPER_EXPORT const char* whisperc_token_string( void* model, int token ) { return ( (iModel*)model )->stringFromToken( token ); }
WHISPER_EXPORT int32_t whisperc_is_multilingual( void* model ) { return ( (iModel*)model )->isMultilingual(); }
// whisper_lang_auto_detect (whisper.cpp:2428-2495) on a mono FP32 16 kHz buffer: probs[ id ] for the first probsCap language ids, *langId = the winner
WHISPER_EXPORT int32_t whisperc_detect_language( void* ctx, const float* pcm, uint32_t nSamples, int32_t offsetMs, float* probs, uint32_t probsCap, int32_t* langId )
{
	if( !ctx || ( !pcm && nSamples ) ) return E_POINTER;
	int id = -1;
	const HRESULT hr = contextDetectLanguage( ctx, pcm, nSamples, offsetMs, probs, probsCap, id );
	if( langId ) *langId = id;
	return hr;
}
// the language the last run (language "auto") or whisperc_detect_language on this context found: code5 receives its code, *p its lang_probs entry
WHISPER_EXPORT int32_t whisperc_detected_language( void* ctx, char* code5, float* p )
{
	if( !ctx ) return E_POINTER;
	float prob = 0;
	const int id = contextDetectedLanguage( ctx, prob );
	if( code5 ) code5[ 0 ] = 0;
	if( p ) *p = 0;
	if( id < 0 ) return S_FALSE;
	if( code5 ) snprintf( code5, 5, "%s", languageCode( id ).c_str() );
	if( p ) *p = prob;
	return S_OK;
}
// of a batch runner's per-stream result: the language the stream was transcribed in when it was detected (language "auto"); S_FALSE otherwise
WHISPER_EXPORT int32_t whisperc_tr_language( void* result, char* code5, float* p )
{
	if( !result ) return E_POINTER;
	if( code5 ) code5[ 0 ] = 0;
	if( p ) *p = 0;
	const TranscribeResult* r = dynamic_cast<const TranscribeResult*>( (iTranscribeResult*)result );
	if( !r || r->languageId < 0 ) return S_FALSE;
	if( code5 ) snprintf( code5, 5, "%s", languageCode( r->languageId ).c_str() );
	if( p ) *p = r->languageP;
	return S_OK;
}
// wh_context_set_flags( flags, parityThreads ) on the device context behind an iContext (tests: WH_FLAG_PARITY_EXACT = 8 makes whisperc_detect_language
// compute the reference's bits). Per context, not process-wide; the greedy loop and beam search refuse the exact mode.
WHISPER_EXPORT int32_t whisperc_debug_context_flags( void* ctx, uint32_t flags, int32_t parityThreads )
{
	if( !ctx ) return E_POINTER;
	return contextSetDeviceFlags( ctx, flags, parityThreads );
}
// Whisper::setDecodingFallback, and Whisper::setBatchDecodingFallback on a runner of whisperc_batch_create
WHISPER_EXPORT int32_t whisperc_set_fallback( void* ctx, int32_t on, float temperatureInc, float logprobThold, float entropyThold, float noSpeechThold, uint64_t seed )
{
	return setFallbackOn<iContext>( &setDecodingFallback, ctx, on, temperatureInc, logprobThold, entropyThold, noSpeechThold, seed );
}
WHISPER_EXPORT int32_t whisperc_batch_set_fallback( void* runner, int32_t on, float temperatureInc, float logprobThold, float entropyThold, float noSpeechThold, uint64_t seed )
{
	return setFallbackOn<iBatchRunner>( &setBatchDecodingFallback, runner, on, temperatureInc, logprobThold, entropyThold, noSpeechThold, seed );
}
// Whisper::getWindowStats: out = sWindowStats [cap] (may be NULL), *count = the windows of the last run
WHISPER_EXPORT int32_t whisperc_window_stats( void* ctx, void* out, uint32_t cap, uint32_t* count )
{
	if( !ctx || !count ) return E_POINTER;
	*count = cap;
	return getWindowStats( (const iContext*)ctx, (sWindowStats*)out, count );
}
// Whisper::getNonSpeechTokens: out = int32 [cap] (may be NULL), *count = the size of the model's non-speech set
WHISPER_EXPORT int32_t whisperc_non_speech_tokens( void* model, int32_t* out, uint32_t cap, uint32_t* count )
{
	if( !model || !count ) return E_POINTER;
	*count = cap;
	return getNonSpeechTokens( (iModel*)model, out, count );
}
// Whisper::setSuppressedTokens / setBatchSuppressedTokens: count == 0 turns suppression off (ids may be NULL)
WHISPER_EXPORT int32_t whisperc_set_suppress_tokens( void* ctx, const int32_t* ids, uint32_t count )
{
	if( !ctx ) return E_POINTER;
	return setSuppressedTokens( (iContext*)ctx, ids, count );
}
WHISPER_EXPORT int32_t whisperc_batch_set_suppress_tokens( void* runner, const int32_t* ids, uint32_t count )
{
	if( !runner ) return E_POINTER;
	return setBatchSuppressedTokens( (iBatchRunner*)runner, ids, count );
}
// Whisper::setBoostedPhrases / setBatchBoostedPhrases / phraseSpellings: count == 0 turns boosting off (the pointers may be NULL)
WHISPER_EXPORT int32_t whisperc_set_boost_phrases( void* ctx, const int32_t* tokens, const int32_t* lens, uint32_t count, uint32_t nMax, float boost )
{
	if( !ctx ) return E_POINTER;
	const sBoostedPhrases p{ tokens, lens, count, nMax, boost };
	return setBoostedPhrases( (iContext*)ctx, count ? &p : nullptr );
}
WHISPER_EXPORT int32_t whisperc_batch_set_boost_phrases( void* runner, const int32_t* tokens, const int32_t* lens, uint32_t count, uint32_t nMax, float boost )
{
	if( !runner ) return E_POINTER;
	const sBoostedPhrases p{ tokens, lens, count, nMax, boost };
	return setBatchBoostedPhrases( (iBatchRunner*)runner, count ? &p : nullptr );
}
WHISPER_EXPORT int32_t whisperc_phrase_spellings( void* model, const char* text, int32_t* tokens, int32_t* lens, uint32_t cap, uint32_t* count )
{
	if( !model || !count ) return E_POINTER;
	*count = cap;
	return phraseSpellings( (iModel*)model, text, tokens, lens, count );
}
// Whisper::setNoRepeatNgram / setBatchNoRepeatNgram: n == 0 turns the rule off
WHISPER_EXPORT int32_t whisperc_set_no_repeat_ngram( void* ctx, int32_t n )
{
	if( !ctx ) return E_POINTER;
	return setNoRepeatNgram( (iContext*)ctx, n );
}
WHISPER_EXPORT int32_t whisperc_batch_set_no_repeat_ngram( void* runner, int32_t n )
{
	if( !runner ) return E_POINTER;
	return setBatchNoRepeatNgram( (iBatchRunner*)runner, n );
}
// Whisper::setSpeechFilter / setBatchSpeechFilter: on == 0 turns the filter off; 0 = a parameter's default
WHISPER_EXPORT int32_t whisperc_set_speech_filter( void* ctx, int32_t on, int32_t minSilenceFrames, int32_t minSpeechFrames, int32_t padFrames )
{
	if( !ctx ) return E_POINTER;
	const sSpeechFilter p{ minSilenceFrames, minSpeechFrames, padFrames, 0 };
	return setSpeechFilter( (iContext*)ctx, on ? &p : nullptr );
}
WHISPER_EXPORT int32_t whisperc_batch_set_speech_filter( void* runner, int32_t on, int32_t minSilenceFrames, int32_t minSpeechFrames, int32_t padFrames )
{
	if( !runner ) return E_POINTER;
	const sSpeechFilter p{ minSilenceFrames, minSpeechFrames, padFrames, 0 };
	return setBatchSpeechFilter( (iBatchRunner*)runner, on ? &p : nullptr );
}
// Whisper::getSpeechSpans / getResultSpeechSpans: out = int64 [cap][2] (may be NULL), *count = the spans the last run / the result's stream used
WHISPER_EXPORT int32_t whisperc_result_speech_spans( void* ctx, int64_t* out, uint32_t cap, uint32_t* count )
{
	if( !ctx || !count ) return E_POINTER;
	*count = cap;
	static_assert( sizeof( sSpeechSpan ) == 16, "sSpeechSpan is two int64" );
	return getSpeechSpans( (const iContext*)ctx, (sSpeechSpan*)out, count );
}
WHISPER_EXPORT int32_t whisperc_tr_speech_spans( void* result, int64_t* out, uint32_t cap, uint32_t* count )
{
	if( !result || !count ) return E_POINTER;
	*count = cap;
	return getResultSpeechSpans( (const iTranscribeResult*)result, (sSpeechSpan*)out, count );
}
// Whisper::setTimestampRules / setBatchTimestampRules
WHISPER_EXPORT int32_t whisperc_set_timestamp_rules( void* ctx, int32_t on )
{
	if( !ctx ) return E_POINTER;
	return setTimestampRules( (iContext*)ctx, on != 0 );
}
WHISPER_EXPORT int32_t whisperc_batch_set_timestamp_rules( void* runner, int32_t on )
{
	if( !runner ) return E_POINTER;
	return setBatchTimestampRules( (iBatchRunner*)runner, on != 0 );
}
// Whisper::getResultWindowStats: out = sWindowStats [cap] (may be NULL), *count = the windows of the result's stream
WHISPER_EXPORT int32_t whisperc_tr_window_stats( void* result, void* out, uint32_t cap, uint32_t* count )
{
	if( !result || !count ) return E_POINTER;
	*count = cap;
	return getResultWindowStats( (const iTranscribeResult*)result, (sWindowStats*)out, count );
}
// Whisper::setAlignmentHeads: count (layer, head) pairs, 0 = the default heads
WHISPER_EXPORT int32_t whisperc_model_set_alignment_heads( void* model, const int32_t* layerHeadPairs, int32_t count )
{
	if( !model ) return E_POINTER;
	if( count < 0 ) return E_INVALIDARG;
	return setAlignmentHeads( (iModel*)model, layerHeadPairs, (uint32_t)count );
}
// the code of language `id` (0 .. 98; the language token is sot + 1 + id): S_FALSE beyond the table
WHISPER_EXPORT int32_t whisperc_language_code( int32_t id, char* code5 )
{
	if( !code5 ) return E_POINTER;
	const std::string code = languageCode( id );
	snprintf( code5, 5, "%s", code.c_str() );
	return code.empty() ? S_FALSE : S_OK;
}
// the host half of whisper_lang_auto_detect on its own (no device): lang_probs from the n probabilities p; returns the winner
WHISPER_EXPORT int32_t whisperc_debug_lang_probs( const float* p, int32_t n, float* probs )
{
	return finishLanguageProbs( p, n, probs );
}
// flags: eFullParamsFlags bits; language: ASCII code; returns the HRESULT of runFull
WHISPER_EXPORT int32_t whisperc_run_full( void* ctx, const float* pcm, uint32_t nSamples, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx )
{
	if( !ctx || ( !pcm && nSamples ) ) return E_POINTER;
	sFullParams p;
	CHECK( fullParams( eSamplingStrategy::Greedy, language, flags, maxTokens, promptTokens, nPrompt, nMaxTextCtx, p ) );
	return runFullOn( ctx, p, pcm, nullptr, nSamples );
}
WHISPER_EXPORT int32_t whisperc_run_full_audio_ctx( void* ctx, const float* pcm, uint32_t nSamples, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, int audioCtx )
{
	if( !ctx || ( !pcm && nSamples ) ) return E_POINTER;
	sFullParams p;
	CHECK( fullParams( eSamplingStrategy::Greedy, language, flags, maxTokens, promptTokens, nPrompt, nMaxTextCtx, p ) );
	p.audio_ctx = audioCtx;
	return runFullOn( ctx, p, pcm, nullptr, nSamples );
}
// initMediaFoundation -> loadAudioFileData( WAV bytes ) -> iContext::runStreamed; progress values are appended to
// progressOut (up to progressCap), their count is returned through progressCount
WHISPER_EXPORT int32_t whisperc_run_streamed( void* ctx, const void* wavBytes, uint64_t wavSize, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, double* progressOut, int progressCap, int* progressCount )
{
	if( !ctx || !wavBytes ) return E_POINTER;
	sFullParams p;
	CHECK( fullParams( eSamplingStrategy::Greedy, language, flags, maxTokens, promptTokens, nPrompt, nMaxTextCtx, p ) );
	iMediaFoundation* mf = nullptr;
	CHECK( initMediaFoundation( &mf ) );
	iAudioReader* reader = nullptr;
	const HRESULT hr = mf->loadAudioFileData( wavBytes, wavSize, false, &reader );
	mf->Release();
	if( FAILED( hr ) ) return hr;
	return runStreamedOn( ctx, p, reader, progressOut, progressCap, progressCount );
}
// whisperc_run_full_range over a buffer that has stereo data: `stereo` = nSamples interleaved frames (2 floats each) of the same recording, what
// iAudioBuffer::getPcmStereo returns; NULL = whisperc_run_full_range. The segments' speakers: whisperc_result_speakers.
WHISPER_EXPORT int32_t whisperc_run_full_stereo( void* ctx, const float* pcm, const float* stereo, uint32_t nSamples, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, int offsetMs, int durationMs )
{
	if( !ctx || ( !pcm && nSamples ) ) return E_POINTER;
	sFullParams p;
	CHECK( fullParams( eSamplingStrategy::Greedy, language, flags, maxTokens, promptTokens, nPrompt, nMaxTextCtx, p ) );
	p.offset_ms = offsetMs;
	p.duration_ms = durationMs;
	return runFullOn( ctx, p, pcm, stereo, nSamples );
}
// whisperc_run_full + sFullParams::offset_ms / duration_ms (the range of the buffer that is transcribed; language "auto" still detects on frame 0)
WHISPER_EXPORT int32_t whisperc_run_full_range( void* ctx, const float* pcm, uint32_t nSamples, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, int offsetMs, int durationMs )
{
	return whisperc_run_full_stereo( ctx, pcm, nullptr, nSamples, language, flags, maxTokens, promptTokens, nPrompt, nMaxTextCtx, offsetMs, durationMs );
}
// iContext::runStreamed over a reader that has stereo data: mono FP32 16 kHz PCM and nSamples interleaved stereo frames of the same recording (NULL: none)
WHISPER_EXPORT int32_t whisperc_run_streamed_stereo( void* ctx, const float* pcm, const float* stereo, uint32_t nSamples, const char* language, uint32_t flags,
	int maxTokens, const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, double* progressOut, int progressCap, int* progressCount )
{
	if( !ctx || ( !pcm && nSamples ) ) return E_POINTER;
	sFullParams p;
	CHECK( fullParams( eSamplingStrategy::Greedy, language, flags, maxTokens, promptTokens, nPrompt, nMaxTextCtx, p ) );
	iAudioReader* reader = nullptr;
	CHECK( createPcmReader( std::vector<float>( pcm, pcm + nSamples ), stereoCopy( stereo, nSamples ), &reader ) );
	return runStreamedOn( ctx, p, reader, progressOut, progressCap, progressCount );
}
// Live capture (Whisper::createPcmCapture, iPcmCapture, iContext::runCapture). durations in seconds, flags: eCaptureFlags (Stereo 1, NoDrop 2)
WHISPER_EXPORT int32_t whisperc_capture_create_rate( float minDuration, float maxDuration, float dropStartSilence, float pauseDuration, uint32_t flags, uint32_t sampleRate,
	void** captureOut )
{
	if( !captureOut ) return E_POINTER;
	sCaptureParams cp;
	cp.minDuration = minDuration;
	cp.maxDuration = maxDuration;
	cp.dropStartSilence = dropStartSilence;
	cp.pauseDuration = pauseDuration;
	cp.flags = flags;
	iPcmCapture* cap = nullptr;
	CHECK( createPcmCaptureAtRate( cp, sampleRate, &cap ) );
	*captureOut = cap;
	return S_OK;
}
WHISPER_EXPORT int32_t whisperc_capture_create( float minDuration, float maxDuration, float dropStartSilence, float pauseDuration, uint32_t flags, void** captureOut )
{
	return whisperc_capture_create_rate( minDuration, maxDuration, dropStartSilence, pauseDuration, flags, 16000, captureOut );
}
WHISPER_EXPORT int32_t whisperc_capture_write( void* capture, const void* samples, int32_t format, int32_t channels, uint32_t frames )
{
	if( !capture ) return E_POINTER;
	return ( (iPcmCapture*)capture )->write( samples, format, channels, frames );
}
WHISPER_EXPORT int32_t whisperc_capture_close( void* capture )
{
	if( !capture ) return E_POINTER;
	return ( (iPcmCapture*)capture )->close();
}
WHISPER_EXPORT uint64_t whisperc_capture_dropped( void* capture )
{
	return capture ? ( (iPcmCapture*)capture )->droppedChunks() : 0;
}
WHISPER_EXPORT void whisperc_capture_destroy( void* capture )
{
	if( capture ) ( (iPcmCapture*)capture )->Release();
}
// iContext::runCapture with the parameters of whisperc_run_full; pfnPiece( pv, startSample, nSamples ) is called behind each piece's job, on the library's
// worker thread, while whisperc_result_* still answer for that piece. Any of the three callbacks may be NULL.
WHISPER_EXPORT int32_t whisperc_run_capture_params( void* ctx, void* capture, const char* language, uint32_t flags, int maxTokens, const int32_t* promptTokens,
	int nPrompt, int nMaxTextCtx, int audioCtx, int beamWidth, int32_t ( *pfnShouldCancelC )( void* ), int32_t ( *pfnCaptureStatusC )( void*, uint8_t ),
	void ( *pfnPiece )( void*, int64_t, int64_t ), void* pv )
{
	if( !ctx ) return E_POINTER;
	sFullParams p;
	CHECK( fullParams( beamWidth > 0 ? eSamplingStrategy::BeamSearch : eSamplingStrategy::Greedy, language, flags, maxTokens, promptTokens, nPrompt, nMaxTextCtx, p ) );
	p.audio_ctx = audioCtx;
	if( beamWidth > 0 ) p.beam_search.beam_width = beamWidth;
	sCaptureCallbacks cb;
	cb.shouldCancel = reinterpret_cast<pfnShouldCancel>( pfnShouldCancelC );
	cb.captureStatus = reinterpret_cast<pfnCaptureStatus>( pfnCaptureStatusC );
	cb.pv = pv;
	return contextRunCapture( ctx, p, cb, (const iPcmCapture*)capture, pfnPiece, pv );
}
WHISPER_EXPORT int32_t whisperc_run_capture( void* ctx, void* capture, const char* language, uint32_t flags, int32_t ( *pfnShouldCancelC )( void* ),
	int32_t ( *pfnCaptureStatusC )( void*, uint8_t ), void ( *pfnPiece )( void*, int64_t, int64_t ), void* pv )
{
	return whisperc_run_capture_params( ctx, capture, language, flags, 0, nullptr, 0, -1, 0, 0, pfnShouldCancelC, pfnCaptureStatusC, pfnPiece, pv );
}
// iContext::detectSpeaker( { t0, t1 } in 100 ns ticks ): *channel = eSpeakerChannel (0 unsure, 1 left, 2 right, 0xFF no stereo data). Outside a run's
// callbacks: OLE_E_BLANK, like the reference.
WHISPER_EXPORT int32_t whisperc_detect_speaker( void* ctx, uint64_t t0, uint64_t t1, uint8_t* channel )
{
	if( !ctx || !channel ) return E_POINTER;
	sTimeInterval time;
	time.begin.ticks = t0;
	time.end.ticks = t1;
	eSpeakerChannel ch = eSpeakerChannel::NoStereoData;
	const HRESULT hr = ( (iContext*)ctx )->detectSpeaker( time, ch );
	*channel = (uint8_t)ch;
	return hr;
}
// Of a transcribe result of this library (iContext::getResults, a batch runner's per-stream result): one eSpeakerChannel byte per segment, what
// iContext::detectSpeaker answered for the segment when it was appended; 0xFF = the run's audio had no stereo data. *count = the segments;
// out may be NULL (count only), cap < *count is E_INVALIDARG.
WHISPER_EXPORT int32_t whisperc_tr_speakers( void* result, uint8_t* out, uint32_t cap, uint32_t* count )
{
	if( !result || !count ) return E_POINTER;
	const ResultData* r = dynamic_cast<const ResultData*>( (iTranscribeResult*)result );
	if( !r ) return E_INVALIDARG;
	const size_t n = r->segments.size();
	*count = (uint32_t)n;
	if( !out ) return S_OK;
	if( cap < n ) return E_INVALIDARG;
	for( size_t i = 0; i < n; i++ ) out[ i ] = i < r->speakers.size() ? r->speakers[ i ] : (uint8_t)0xFF;
	return S_OK;
}
// the same of a context's results (iContext::getResults)
WHISPER_EXPORT int32_t whisperc_result_speakers( void* ctx, uint8_t* out, uint32_t cap, uint32_t* count )
{
	if( !ctx ) return E_POINTER;
	iTranscribeResult* r = nullptr;
	CHECK( ( (iContext*)ctx )->getResults( eResultFlags::Timestamps, &r ) );
	return whisperc_tr_speakers( r, out, cap, count );
}
// wh_resample_host behind an HRESULT: *nOut = the 16 kHz samples the input gives; dst == NULL only counts, cap < *nOut is E_INVALIDARG
WHISPER_EXPORT int32_t whisperc_resample( const void* src, int32_t format, int32_t channels, int32_t channel, int32_t rate, int64_t nFrames, float* dst, int64_t cap,
	int64_t* nOut )
{
	if( !nOut || ( !src && nFrames > 0 ) ) return E_POINTER;
	if( format < 0 || format > 4 || channels < 1 || channels > 8 || channel < -1 || channel >= channels ) return E_INVALIDARG;
	if( 0 != wh_resample_out_len( rate, nFrames, nOut ) ) return E_INVALIDARG;
	if( !dst ) return S_OK;
	if( cap < *nOut ) return E_INVALIDARG;
	CHECK_WH( wh_resample_host( src, format, channels, channel, rate, nFrames, dst, 1, *nOut ) );
	return S_OK;
}
// iMediaFoundation::loadAudioFile + iAudioBuffer::getPcmMono / getPcmStereo: *nFrames = the 16 kHz frames of the file; dst == NULL reads the file and parses its
// chunks (the `data` chunk's clipped length needs the file's size) but converts nothing
WHISPER_EXPORT int32_t whisperc_load_audio( const char* pathUtf8, int32_t stereo, float* dst, int64_t cap, int64_t* nFrames )
{
	if( !pathUtf8 || !nFrames ) return E_POINTER;
	if( !dst )
	{
		std::ifstream f( pathUtf8, std::ios::binary );
		if( !f ) { logError( "failed to open audio file '%s'", pathUtf8 ); return (HRESULT)0x80070002; }
		std::vector<char> data( ( std::istreambuf_iterator<char>( f ) ), std::istreambuf_iterator<char>() );
		wav::Info info;
		std::string error;
		if( !wav::parse( data.data(), data.size(), info, error ) ) { logError( "'%s': %s", pathUtf8, error.c_str() ); return E_INVALIDARG; }
		return 0 == wh_resample_out_len( info.rate, (int64_t)info.frames, nFrames ) ? S_OK : E_INVALIDARG;
	}
	iMediaFoundation* mf = nullptr;
	CHECK( initMediaFoundation( &mf ) );
	iAudioBuffer* buf = nullptr;
	const HRESULT hr = mf->loadAudioFile( pathUtf8, stereo != 0, &buf );
	mf->Release();
	if( FAILED( hr ) ) return hr;
	const int64_t n = buf->countSamples(), floats = stereo ? 2 * n : n;
	*nFrames = n;
	HRESULT res = S_OK;
	if( cap < floats ) res = E_INVALIDARG;
	else if( n > 0 && stereo && !buf->getPcmStereo() )
	{
		// a mono file: the buffer has no stereo data (iContext::detectSpeaker answers NoStereoData for it); this entry point hands out the one channel twice
		const float* const m = buf->getPcmMono();
		for( int64_t i = 0; i < n; i++ ) dst[ 2 * i ] = dst[ 2 * i + 1 ] = m[ i ];
	}
	else if( n > 0 ) memcpy( dst, stereo ? buf->getPcmStereo() : buf->getPcmMono(), (size_t)floats * sizeof( float ) );
	buf->Release();
	return res;
}
// iContext::fullDefaultParams( BeamSearch ) + beam_search.beam_width = beamWidth (1 .. 8), then iContext::runFull
WHISPER_EXPORT int32_t whisperc_run_full_beam( void* ctx, const float* pcm, uint32_t nSamples, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, int beamWidth )
{
	if( !ctx || ( !pcm && nSamples ) ) return E_POINTER;
	sFullParams p;
	CHECK( fullParams( eSamplingStrategy::BeamSearch, language, flags, maxTokens, promptTokens, nPrompt, nMaxTextCtx, p ) );
	p.beam_search.beam_width = beamWidth;
	return runFullOn( ctx, p, pcm, nullptr, nSamples );
}
// whisperc_run_full with the token-timestamp parameters of sFullParams (thold_pt, thold_ptsum, max_len; sFullParams.h:79-86)
WHISPER_EXPORT int32_t whisperc_run_full_tt( void* ctx, const float* pcm, uint32_t nSamples, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, float tholdPt, float tholdPtsum, int maxLen )
{
	if( !ctx || ( !pcm && nSamples ) ) return E_POINTER;
	sFullParams p;
	CHECK( fullParams( eSamplingStrategy::Greedy, language, flags, maxTokens, promptTokens, nPrompt, nMaxTextCtx, p ) );
	p.thold_pt = tholdPt;
	p.thold_ptsum = tholdPtsum;
	p.max_len = maxLen;
	return runFullOn( ctx, p, pcm, nullptr, nSamples );
}
// Copies the results out: of a context's results (whisperc_result_*), of a transcribe result (whisperc_tr_*: a batch runner's per-stream result)
WHISPER_EXPORT int32_t whisperc_result_counts( void* ctx, uint32_t* segments, uint32_t* tokens )
{
	iTranscribeResult* r = nullptr;
	CHECK( contextResults( ctx, r ) );
	return resultCounts( r, segments, tokens );
}
WHISPER_EXPORT int32_t whisperc_result_segment( void* ctx, uint32_t index, uint64_t* t0, uint64_t* t1, uint32_t* firstToken, uint32_t* countTokens,
	char* text, uint32_t textCap )
{
	iTranscribeResult* r = nullptr;
	CHECK( contextResults( ctx, r ) );
	return resultSegment( r, index, t0, t1, firstToken, countTokens, text, textCap );
}
WHISPER_EXPORT int32_t whisperc_result_token( void* ctx, uint32_t index, int32_t* id, float* p, float* pt, float* ptsum )
{
	iTranscribeResult* r = nullptr;
	CHECK( contextResults( ctx, r ) );
	const sToken* t = nullptr;
	CHECK( resultToken( r, index, t ) );
	*id = t->id; *p = t->probability; *pt = t->probabilityTimestamp; *ptsum = t->ptsum;
	return S_OK;
}
WHISPER_EXPORT int32_t whisperc_result_token_times( void* ctx, uint32_t index, uint64_t* t0, uint64_t* t1, float* vlen )
{
	iTranscribeResult* r = nullptr;
	CHECK( contextResults( ctx, r ) );
	const sToken* t = nullptr;
	CHECK( resultToken( r, index, t ) );
	*t0 = t->time.begin.ticks; *t1 = t->time.end.ticks; *vlen = t->vlen;
	return S_OK;
}
WHISPER_EXPORT int32_t whisperc_tr_counts( void* result, uint32_t* segments, uint32_t* tokens )
{
	return resultCounts( (iTranscribeResult*)result, segments, tokens );
}
WHISPER_EXPORT int32_t whisperc_tr_segment( void* result, uint32_t index, uint64_t* t0, uint64_t* t1, uint32_t* firstToken, uint32_t* countTokens, char* text, uint32_t textCap )
{
	return resultSegment( (iTranscribeResult*)result, index, t0, t1, firstToken, countTokens, text, textCap );
}
WHISPER_EXPORT int32_t whisperc_tr_token( void* result, uint32_t index, int32_t* id, float* p, float* pt, float* ptsum, uint64_t* t0, uint64_t* t1, float* vlen )
{
	const sToken* t = nullptr;
	CHECK( resultToken( (iTranscribeResult*)result, index, t ) );
	*id = t->id; *p = t->probability; *pt = t->probabilityTimestamp; *ptsum = t->ptsum;
	*t0 = t->time.begin.ticks; *t1 = t->time.end.ticks; *vlen = t->vlen;
	return S_OK;
}
WHISPER_EXPORT int32_t whisperc_tokenize( void* model, const char* text, int32_t* out, int cap )
{
	struct Sink { int32_t* out; int cap; int n; } sink{ out, cap, 0 };
	const HRESULT hr = ( (iModel*)model )->tokenize( text, []( const int* toks, int n, void* pv ) {
		Sink* s = (Sink*)pv;
		s->n = n;
		for( int i = 0; i < n && i < s->cap; i++ ) s->out[ i ] = toks[ i ];
	}, &sink );
	return FAILED( hr ) ? hr : sink.n;
}
WHISPER_EXPORT int32_t whisperc_timings_print( void* ctx ) { return ( (iContext*)ctx )->timingsPrint(); }

// ---- the lock-step batch runner (Whisper::createBatchRunner / iBatchRunner::run) for FFI callers ----
namespace
{
	// a caller's PCM as an iAudioBuffer without a copy; the memory stays the caller's for the duration of the call. Declared inside the extern "C" block:
	// g++ then puts the class's type information (_ZTIN12_GLOBAL__N_17PcmViewE) into libWhisper.so's dynamic symbols, and that list is part of the boundary.
	class PcmView : public ComObject<iAudioBuffer>
	{
		const float* const pcm;
		const float* const stereo;	   // n interleaved frames, or nullptr
		const uint32_t n;
	public:
		PcmView( const float* p, const float* st, uint32_t count ) : pcm( p ), stereo( st ), n( count ) {}
		uint32_t countSamples() const override { return n; }
		const float* getPcmMono() const override { return n ? pcm : nullptr; }
		const float* getPcmStereo() const override { return n ? stereo : nullptr; }
		HRESULT getTime( int64_t& rdi ) const override { rdi = 0; return S_OK; }
	};
}
WHISPER_EXPORT int32_t whisperc_batch_create( void* model, uint32_t maxSlots, uint32_t groups, uint32_t greedyChunk, uint32_t flags, void** runnerOut )
{
	if( !model || !runnerOut ) return E_POINTER;
	const sBatchSetup setup{ maxSlots, groups, greedyChunk, flags };
	iBatchRunner* r = nullptr;
	const HRESULT hr = createBatchRunner( (iModel*)model, &setup, &r );
	*runnerOut = r;
	return hr;
}
// whisperc_batch_run over buffers that have stereo data: stereo[i] = nSamples[i] interleaved frames of the recording pcm[i] is the mono of, or NULL
// (stereo itself may be NULL: whisperc_batch_run). Every result carries its segments' speakers (whisperc_tr_speakers).
WHISPER_EXPORT int32_t whisperc_batch_run_stereo( void* runner, uint32_t count, const float* const* pcm, const float* const* stereo, const uint32_t* nSamples,
	const int64_t* firstSample, const int64_t* countSamples, const char* language, uint32_t flags, int maxTokens, const int32_t* promptTokens, int nPrompt,
	int nMaxTextCtx, void** resultsOut, int32_t* perStream )
{
	if( !runner || !resultsOut || ( count && ( !pcm || !nSamples ) ) ) return E_POINTER;
	sFullParams p;
	CHECK( fullParams( eSamplingStrategy::Greedy, language, flags, maxTokens, promptTokens, nPrompt, nMaxTextCtx, p ) );
	// one view per distinct buffer: the chunks of a recording share it
	std::map<std::pair<std::pair<const float*, const float*>, uint32_t>, PcmView*> views;
	std::vector<sBatchStream> streams( count );
	for( uint32_t i = 0; i < count; i++ )
	{
		const float* const st = stereo ? stereo[ i ] : nullptr;
		PcmView*& v = views[ { { pcm[ i ], st }, nSamples[ i ] } ];
		if( !v ) v = new PcmView( pcm[ i ], st, nSamples[ i ] );
		streams[ i ] = sBatchStream{ v, firstSample ? firstSample[ i ] : 0, countSamples ? countSamples[ i ] : 0, nullptr };
	}
	std::vector<iTranscribeResult*> res( count, nullptr );
	static_assert( sizeof( HRESULT ) == sizeof( int32_t ), "HRESULT" );
	const HRESULT hr = ( (iBatchRunner*)runner )->run( p, streams.data(), count, res.data(), perStream );
	for( uint32_t i = 0; i < count; i++ ) resultsOut[ i ] = res[ i ];
	for( auto& kv : views ) kv.second->Release();
	return hr;
}
WHISPER_EXPORT int32_t whisperc_batch_run( void* runner, uint32_t count, const float* const* pcm, const uint32_t* nSamples, const int64_t* firstSample,
	const int64_t* countSamples, const char* language, uint32_t flags, int maxTokens, const int32_t* promptTokens, int nPrompt, int nMaxTextCtx,
	void** resultsOut, int32_t* perStream )
{
	return whisperc_batch_run_stereo( runner, count, pcm, nullptr, nSamples, firstSample, countSamples, language, flags, maxTokens, promptTokens, nPrompt, nMaxTextCtx,
		resultsOut, perStream );
}
// Host-only post-processing of token data into token times, on its own (no device): what runFull does per segment under the
// TokenTimestamps flag. Segments are processed in order (the anchors carry state from one to the next).
WHISPER_EXPORT int32_t whisperc_debug_token_timestamps( const char* modelPath, const float* pcm, uint64_t nSamples, int32_t nSegments,
	const int64_t* segTimes, const int32_t* segTokenCounts, const int32_t* ids, const int32_t* tids, const float* p, const float* pt,
	const float* ptsum, float tholdPt, float tholdPtsum, int32_t maxLen, int32_t segCap, int32_t tokCap, int32_t* outSegCount,
	int64_t* outSegTimes, int32_t* outSegTokenCounts, char* outTexts, uint32_t textCap, int64_t* outTokTimes, float* outVlen )
{
	if( !modelPath || !pcm || !segTimes || !segTokenCounts || !ids || !tids || !p || !pt || !ptsum || !outSegCount ) return E_POINTER;
	Vocabulary vocab;
	const HRESULT hr = loadVocabulary( modelPath, vocab );
	if( FAILED( hr ) ) return hr;
	TokenTimestamper stamper;
	stamper.begin( pcm, (size_t)nSamples );
	std::vector<Segment> all;
	size_t at = 0;
	for( int i = 0; i < nSegments; i++ )
	{
		Segment s;
		s.t0 = segTimes[ 2 * i ]; s.t1 = segTimes[ 2 * i + 1 ];
		for( int j = 0; j < segTokenCounts[ i ]; j++, at++ )
		{
			TokenData t;
			t.id = ids[ at ]; t.tid = tids[ at ]; t.p = p[ at ]; t.pt = pt[ at ]; t.ptsum = ptsum[ at ];
			s.tokens.push_back( t );
			if( t.id < vocab.token_eot && vocab.string( t.id ) ) s.text += vocab.string( t.id );
		}
		all.push_back( std::move( s ) );
		stamper.compute( all.back(), vocab, tholdPt, tholdPtsum );
		if( maxLen > 0 ) TokenTimestamper::wrapLast( all, vocab, maxLen );
	}
	size_t nTok = 0, textAt = 0;
	for( const Segment& s : all ) nTok += s.tokens.size();
	if( (int)all.size() > segCap || (int)nTok > tokCap ) return E_BOUNDS;
	*outSegCount = (int32_t)all.size();
	size_t k = 0;
	for( size_t i = 0; i < all.size(); i++ )
	{
		const Segment& s = all[ i ];
		outSegTimes[ 2 * i ] = s.t0; outSegTimes[ 2 * i + 1 ] = s.t1;
		outSegTokenCounts[ i ] = (int32_t)s.tokens.size();
		if( textAt + s.text.size() + 1 > textCap ) return E_BOUNDS;
		memcpy( outTexts + textAt, s.text.c_str(), s.text.size() + 1 );	   // NUL-separated
		textAt += s.text.size() + 1;
		for( const TokenData& t : s.tokens )
		{
			outTokTimes[ 2 * k ] = t.t0; outTokTimes[ 2 * k + 1 ] = t.t1;
			outVlen[ k ] = t.vlen;
			k++;
		}
	}
	return S_OK;
}
// Vocabulary + tokenizer of a model file on their own (host only): what iModel::tokenize / stringFromToken / getSpecialTokens answer
WHISPER_EXPORT int32_t whisperc_debug_tokenize( const char* modelPath, const char* text, int32_t* out, int cap )
{
	if( !modelPath || !text || ( !out && cap > 0 ) ) return E_POINTER;
	Vocabulary vocab;
	const HRESULT hr = loadVocabulary( modelPath, vocab );
	if( FAILED( hr ) ) return hr;
	std::vector<int> toks;
	const HRESULT hr2 = vocab.tokenize( text, toks );
	if( FAILED( hr2 ) ) return hr2;
	if( (int)toks.size() > cap ) return E_BOUNDS;
	for( size_t i = 0; i < toks.size(); i++ ) out[ i ] = toks[ i ];
	return (int32_t)toks.size();
}
// Whisper::phraseSpellings on the vocabulary of a model file (host only): the arguments of whisperc_phrase_spellings
WHISPER_EXPORT int32_t whisperc_debug_phrase_spellings( const char* modelPath, const char* text, int32_t* tokens, int32_t* lens, uint32_t cap, uint32_t* count )
{
	if( !modelPath || !count ) return E_POINTER;
	Vocabulary vocab;
	const HRESULT hr = loadVocabulary( modelPath, vocab );
	if( FAILED( hr ) ) return hr;
	*count = cap;
	return phraseSpellingsOf( vocab, text, tokens, lens, count );
}
WHISPER_EXPORT int32_t whisperc_debug_token_string( const char* modelPath, int32_t token, char* out, uint32_t outCap, int32_t* specials8 )
{
	if( !modelPath || !out || outCap == 0 ) return E_POINTER;
	Vocabulary vocab;
	const HRESULT hr = loadVocabulary( modelPath, vocab );
	if( FAILED( hr ) ) return hr;
	const char* const str = vocab.string( token );
	snprintf( out, outCap, "%s", str ? str : "" );
	if( specials8 )
	{
		const int v[ 8 ] = { vocab.token_eot, vocab.token_sot, vocab.token_prev, vocab.token_solm, vocab.token_not, vocab.token_beg,
			vocab.token_translate, vocab.token_transcribe };
		for( int i = 0; i < 8; i++ ) specials8[ i ] = v[ i ];
	}
	return str ? S_OK : S_FALSE;
}
WHISPER_EXPORT int32_t whisperc_format_measure( const char* name, double ticks, uint64_t count, char* out, uint32_t outCap )
{
	if( !name || !out || outCap == 0 ) return -1;
	const std::string s = formatMeasure( name, ticks, count );
	const size_t n = std::min( s.size(), (size_t)outCap - 1 );
	memcpy( out, s.data(), n );
	out[ n ] = 0;
	return (int32_t)n;
}
WHISPER_EXPORT int32_t whisperc_set_beam_ranking( int onHost )
{
	if( onHost != 0 && onHost != 1 ) return E_INVALIDARG;
	setBeamRankingOnHost( onHost != 0 );
	return S_OK;
}
WHISPER_EXPORT int32_t whisperc_set_host_loop_rules( int mode )
{
	if( mode != 0 && mode != 1 ) return E_INVALIDARG;
	g_hostLoopRules = (eHostLoopRules)mode;
	return S_OK;
}
}
