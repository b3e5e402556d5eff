// One long recording onto the batched path: voice-activity features on the device (wh_vad_features), the reference's decision loop over them (vad.h) and
// the chunk planner (chunkPlanner.h). Whisper::splitAtPauses of whisperApi.h and its flat C mirror (whisper_c.h). Whisper::speechSpans, the spans of the
// speech filter alone (speechSpans.h), takes the same way to the flags.
//
// Known cost: the PCM goes to the device twice -- once here for the features, once per chunk by the batch runner's admission (12.8 MB for 200 s).
#include "hostCommon.h"
#include "chunkPlanner.h"
#include "optionRules.h"
#include <cstring>

namespace Whisper
{
	namespace
	{
		// features on the calling thread's current device, then the decision: flags and energies of the N / 256 whole frames
		HRESULT detect( const float* pcm, int64_t nSamples, std::vector<uint8_t>& speech, std::vector<float>& energy, int64_t& lastSpeech )
		{
			int64_t nFrames = 0;
			if( nSamples < 0 || 0 != wh_vad_frame_count( nSamples, &nFrames ) ) return E_INVALIDARG;
			if( nFrames > 0 && !pcm ) return E_POINTER;
			std::vector<float> feat( (size_t)nFrames * 3 );
			CHECK_WH( wh_vad_features_host( pcm, nSamples, feat.data() ) );
			speech.assign( (size_t)nFrames, 0 );
			lastSpeech = vad::decide( feat.data(), nFrames, speech.data() );
			energy.resize( (size_t)nFrames );
			for( int64_t i = 0; i < nFrames; i++ ) energy[ (size_t)i ] = feat[ (size_t)i * 3 ];
			return S_OK;
		}

		HRESULT planFor( const float* pcm, int64_t nSamples, int64_t maxLen, int64_t minLen, int64_t pauseFrames, std::vector<chunkPlanner::Chunk>& chunks )
		{
			// refuse bad parameters before the device is asked for anything
			int64_t a = maxLen, b = minLen, c = pauseFrames;
			CHECK( chunkPlanner::resolveParams( a, b, c ) );
			std::vector<uint8_t> speech;
			std::vector<float> energy;
			int64_t lastSpeech = 0;
			if( nSamples > a ) CHECK( detect( pcm, nSamples, speech, energy, lastSpeech ) );
			else
			{
				// one chunk whatever the samples are: no device work
				if( nSamples < 0 ) return E_INVALIDARG;
				speech.assign( (size_t)( nSamples / vad::FRAME_SAMPLES ), 0 );
				energy.assign( speech.size(), 0.0f );
			}
			return chunkPlanner::plan( speech.data(), energy.data(), (int64_t)speech.size(), nSamples, maxLen, minLen, pauseFrames, chunks );
		}
	}

	// the spans a run with these parameters transcribes: the same features, decision and rules as wh_context_speech_filter applies on a context's stream
	static HRESULT spansFor( const float* pcm, int64_t nSamples, const sSpeechFilter* params, std::vector<sSpeechSpan>& out )
	{
		const sSpeechFilter defaults{ 0, 0, 0, 0 };
		const sSpeechFilter& p = params ? *params : defaults;
		// refuse bad parameters before the device is asked for anything
		CHECK( optionRules::checkSpeechFilter( "speechSpans", p ) );
		std::vector<uint8_t> speech;
		std::vector<float> energy;
		int64_t lastSpeech = 0;
		CHECK( detect( pcm, nSamples, speech, energy, lastSpeech ) );
		std::vector<speechRules::Span> spans;
		CHECK( speechRules::find( speech.data(), (int64_t)speech.size(), nSamples, p.minSilenceFrames, p.minSpeechFrames, p.padFrames, spans ) );
		out.clear();
		for( const speechRules::Span& s : spans ) out.push_back( sSpeechSpan{ s.a, s.b } );
		return S_OK;
	}
	HRESULT speechSpans( const iAudioBuffer* buffer, const sSpeechFilter* params, pfnSpeechSpans pfnSpans, void* pv )
	{
		if( !buffer || !pfnSpans ) return E_POINTER;
		std::vector<sSpeechSpan> spans;
		CHECK( spansFor( buffer->getPcmMono(), (int64_t)buffer->countSamples(), params, spans ) );
		return pfnSpans( spans.data(), (uint32_t)spans.size(), pv );
	}

	HRESULT splitAtPauses( const iAudioBuffer* buffer, const sSplitParams* params, pfnSplitChunks pfnChunks, void* pv )
	{
		if( !buffer || !pfnChunks ) return E_POINTER;
		const sSplitParams defaults{ 0, 0, 0, 0 };
		const sSplitParams& p = params ? *params : defaults;
		std::vector<chunkPlanner::Chunk> chunks;
		CHECK( planFor( buffer->getPcmMono(), (int64_t)buffer->countSamples(), p.maxLen, p.minLen, (int64_t)p.pauseFrames, chunks ) );
		std::vector<sBatchStream> streams;
		streams.reserve( chunks.size() );
		for( const auto& c : chunks ) streams.push_back( sBatchStream{ buffer, c.firstSample, c.countSamples, nullptr } );
		return pfnChunks( streams.data(), (uint32_t)streams.size(), pv );
	}
}

using namespace Whisper;

extern "C" {

// wh_vad_features_host + vad::decide: *nFrames = nSamples / 256; speech == NULL only counts (no device work), cap < *nFrames is E_INVALIDARG
WHISPER_EXPORT int32_t whisperc_vad( const float* pcm, int64_t nSamples, uint8_t* speech, int64_t cap, int64_t* nFrames, int64_t* lastSpeech )
{
	if( !nFrames ) return E_POINTER;
	if( nSamples < 0 || 0 != wh_vad_frame_count( nSamples, nFrames ) ) return E_INVALIDARG;
	if( !speech ) return S_OK;
	if( cap < *nFrames ) return E_INVALIDARG;
	std::vector<uint8_t> flags;
	std::vector<float> energy;
	int64_t last = 0;
	CHECK( detect( pcm, nSamples, flags, energy, last ) );
	if( !flags.empty() ) memcpy( speech, flags.data(), flags.size() );
	if( lastSpeech ) *lastSpeech = last;
	return S_OK;
}

// the plan of splitAtPauses for a bare PCM buffer: *nChunks = the chunks; first / count may be NULL (count only), cap < *nChunks is E_INVALIDARG
WHISPER_EXPORT int32_t whisperc_plan_chunks( const float* pcm, int64_t nSamples, int64_t maxLen, int64_t minLen, int32_t pauseFrames, int64_t* first, int64_t* count,
	int32_t cap, int32_t* nChunks )
{
	if( !nChunks ) return E_POINTER;
	if( pauseFrames < 0 ) return E_INVALIDARG;
	std::vector<chunkPlanner::Chunk> chunks;
	CHECK( planFor( pcm, nSamples, maxLen, minLen, pauseFrames, chunks ) );
	*nChunks = (int32_t)chunks.size();
	if( !first || !count ) return S_OK;
	if( cap < *nChunks ) return E_INVALIDARG;
	for( size_t i = 0; i < chunks.size(); i++ )
	{
		first[ i ] = chunks[ i ].firstSample;
		count[ i ] = chunks[ i ].countSamples;
	}
	return S_OK;
}

// Whisper::speechSpans for a bare PCM buffer: *count = the spans; spans = int64 [cap][2] or NULL (count only), cap < *count is E_BOUNDS. 0 = a parameter's default
WHISPER_EXPORT int32_t whisperc_speech_spans( const float* pcm, int64_t nSamples, int32_t minSilenceFrames, int32_t minSpeechFrames, int32_t padFrames, int64_t* spans,
	uint32_t cap, uint32_t* count )
{
	if( !count ) return E_POINTER;
	const sSpeechFilter p{ minSilenceFrames, minSpeechFrames, padFrames, 0 };
	std::vector<sSpeechSpan> all;
	CHECK( spansFor( pcm, nSamples, &p, all ) );
	*count = (uint32_t)all.size();
	if( !spans ) return S_OK;
	if( cap < all.size() ) return E_BOUNDS;
	for( size_t i = 0; i < all.size(); i++ ) { spans[ 2 * i ] = all[ i ].firstSample; spans[ 2 * i + 1 ] = all[ i ].endSample; }
	return S_OK;
}

// the host half on its own (no device): vad::decide over nFrames x ( energy, F, SFM )
WHISPER_EXPORT int32_t whisperc_debug_vad_decide( const float* feat, int64_t nFrames, uint8_t* speech, int64_t* lastSpeech )
{
	if( nFrames < 0 ) return E_INVALIDARG;
	if( nFrames > 0 && !feat ) return E_POINTER;
	const int64_t last = vad::decide( feat, nFrames, speech );
	if( lastSpeech ) *lastSpeech = last;
	return S_OK;
}

}	// extern "C"
