// iTranscribeResult of the library: segments + tokens in the reference's POD layout (Whisper/Whisper/TranscribeResult.h), filled from
// the transcript a stream built (hostLoop.h). Shared by iContext::getResults and Whisper::runFullBatch.
#pragma once
#include "hostCommon.h"
#include "hostLoop.h"
#include "diarize.h"

namespace Whisper
{
	struct ResultData
	{
		std::vector<sSegment> segments;
		std::vector<sToken> tokens;
		std::vector<std::string> texts;
		// eSpeakerChannel per segment of a run over stereo audio, what iContext::detectSpeaker answered for the segment's times when it was appended
		// (whisperc_tr_speakers reads them); 0xFF = NoStereoData. Beside the segments, not in them: sSegment is the reference's POD.
		std::vector<uint8_t> speakers;
	};
	class TranscribeResult : public ComObject<iTranscribeResult>, public ResultData
	{
	public:
		// a batch runner's stream whose language was detected (language "auto"): its id and lang_probs entry; -1 = the language was named.
		// Plain members behind the interface's methods: the vtable is the reference's (whisperc_tr_language reads them).
		int languageId = -1;
		float languageP = 0;
		// a batch runner's stream with Whisper::setBatchDecodingFallback on: what the fallback did with each of its windows (getResultWindowStats reads them)
		std::vector<sWindowStats> windowStats;
		// a batch runner's stream with Whisper::setBatchSpeechFilter on: the spans it was transcribed from, relative to its first sample (getResultSpeechSpans reads them)
		std::vector<sSpeechSpan> spans;
		HRESULT getSize( sTranscribeLength& rdi ) const override
		{
			rdi.countSegments = (uint32_t)segments.size();
			rdi.countTokens = (uint32_t)tokens.size();
			return S_OK;
		}
		const sSegment* getSegments() const override { return segments.empty() ? nullptr : segments.data(); }
		const sToken* getTokens() const override { return tokens.empty() ? nullptr : tokens.data(); }
	};

	// The object EMBEDDED in a context: handed out by getResults without eResultFlags::NewObject, it lives as long as the context and its
	// Release never deletes (Whisper/Whisper/TranscribeResult.h:34-43, ContextImpl.misc.cpp:203-209): the idiomatic
	// `CComPtr<iTranscribeResult> r; ctx->getResults( flags, &r );` of a callback (Examples/main/main.cpp:57-58) releases it on scope exit.
	class TranscribeResultStatic : public iTranscribeResult, public ResultData
	{
	public:
		HRESULT QueryInterface( const ComLight::GUID& riid, void** ppv ) override
		{
			if( !ppv ) return E_POINTER;
			if( riid == iTranscribeResult::iid() || riid == ComLight::IID_IUnknown ) { *ppv = this; return S_OK; }
			return E_NOINTERFACE;
		}
		uint32_t AddRef() override { return 1; }
		uint32_t Release() override { return 1; }
		HRESULT getSize( sTranscribeLength& rdi ) const override
		{
			rdi.countSegments = (uint32_t)segments.size();
			rdi.countTokens = (uint32_t)tokens.size();
			return S_OK;
		}
		const sSegment* getSegments() const override { return segments.empty() ? nullptr : segments.data(); }
		const sToken* getTokens() const override { return tokens.empty() ? nullptr : tokens.data(); }
	};

	// The speakers of the segments appended since the last call (speakers.size() .. resultAll.size()), at the moment new_segment fires for them: the
	// reference's rule (diarize.h) on the times getResults reports. stereo == nullptr: the run's audio has no stereo data, every segment is 0xFF; so is a
	// segment that starts past the end of the stereo data (E_BOUNDS: there is no data to judge it by).
	inline void appendSpeakers( const std::vector<Segment>& resultAll, int64_t mediaTimeOffset, const float* stereo, size_t frames, std::vector<uint8_t>& speakers )
	{
		if( speakers.size() > resultAll.size() ) speakers.clear();
		for( size_t i = speakers.size(); i < resultAll.size(); i++ )
		{
			eSpeakerChannel ch = eSpeakerChannel::NoStereoData;
			if( stereo )
			{
				sTimeInterval time;
				time.begin.ticks = (uint64_t)( resultAll[ i ].t0 * 100000 + resultAll[ i ].shift0 + mediaTimeOffset );
				time.end.ticks = (uint64_t)( resultAll[ i ].t1 * 100000 + resultAll[ i ].shift1 + mediaTimeOffset );
				if( FAILED( diarize::detectSpeaker( stereo, frames, mediaTimeOffset, time, ch ) ) ) ch = eSpeakerChannel::NoStereoData;
			}
			speakers.push_back( (uint8_t)ch );
		}
	}

	// Segment times: 10 ms units -> 100 ns ticks, plus the segment's own shift (a stream with a time map, hostLoop.h; 0 otherwise), plus the media time of the first sample (ContextImpl.misc.cpp getResults)
	inline HRESULT fillResultData( const std::vector<Segment>& resultAll, const Vocabulary& vocab, int64_t mediaTimeOffset, eResultFlags flags, ResultData& res )
	{
		const bool withTokens = flags & eResultFlags::Tokens, withTimes = flags & eResultFlags::Timestamps;
		res.segments.resize( resultAll.size() );
		res.texts.resize( resultAll.size() );
		size_t tc = 0;
		if( withTokens )
			for( const Segment& s : resultAll ) tc += s.tokens.size();
		res.tokens.resize( tc );
		size_t soFar = 0;
		auto ticks = []( int64_t t10ms ) { return (uint64_t)( t10ms * 100000 ); };	 // 10 ms -> 100 ns
		// A token whose times were never computed (no TokenTimestamps flag) reports 0. Under the GPU model's rules a token's times START
		// at 0 instead of "unknown" (hostLoop.h), so makeResults reports the media time for it (ContextImpl.misc.cpp:277-283); pinned on
		// the reference's own makeResults, tests/golden/ref_hostloop_contextimpl.json "results".
		const bool fromZero = g_hostLoopRules == eHostLoopRules::ContextImpl;
		auto tokenTicks = [ & ]( int64_t t10ms, int64_t shift ) -> uint64_t
		{
			if( !withTimes || ( t10ms < 0 && !fromZero ) ) return 0;
			return ticks( std::max<int64_t>( t10ms, 0 ) ) + (uint64_t)shift + (uint64_t)mediaTimeOffset;
		};
		for( size_t i = 0; i < resultAll.size(); i++ )
		{
			const Segment& src = resultAll[ i ];
			sSegment& dst = res.segments[ i ];
			res.texts[ i ] = src.text;
			dst.text = res.texts[ i ].c_str();
			dst.time.begin.ticks = withTimes ? ticks( src.t0 ) + (uint64_t)src.shift0 + (uint64_t)mediaTimeOffset : 0;
			dst.time.end.ticks = withTimes ? ticks( src.t1 ) + (uint64_t)src.shift1 + (uint64_t)mediaTimeOffset : 0;
			dst.firstToken = (uint32_t)soFar;
			dst.countTokens = (uint32_t)src.tokens.size();
			if( withTokens )
				for( size_t j = 0; j < src.tokens.size(); j++ )
				{
					const TokenData& t = src.tokens[ j ];
					sToken& o = res.tokens[ soFar + j ];
					o.text = vocab.string( t.id );
					o.time.begin.ticks = tokenTicks( t.t0, t.shift0 );
					o.time.end.ticks = tokenTicks( t.t1, t.shift1 );
					o.probability = t.p; o.probabilityTimestamp = t.pt; o.ptsum = t.ptsum; o.vlen = t.vlen;
					o.id = t.id;
					o.flags = t.id >= vocab.token_eot ? eTokenFlags::Special : eTokenFlags::None;
				}
			soFar += src.tokens.size();
		}
		return S_OK;
	}
}
