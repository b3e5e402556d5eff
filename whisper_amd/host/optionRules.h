// The decoding options of whisperApi.h that are functions over an iContext or an iBatchRunner instead of methods (fallback, suppressed tokens, timestamp rules,
// boosted phrases, no-repeat n-grams, scoring): what the two share, stated once. Host only and header only, no device symbol is named -- ContextImpl (whisperImpl.cpp) and
// BatchRunner (batchScheduler.cpp, which is also compiled into CPU test libraries) both call it. `name` is the public function's, for the log:
// "setSuppressedTokens: ..." against "setBatchSuppressedTokens: ...".
#pragma once
#include "hostCommon.h"
#include "phraseBoost.h"
#include "speechSpans.h"
#include <cmath>

namespace Whisper
{
	namespace optionRules
	{
		inline HRESULT checkFallback( const char* name, const sDecodingFallback& p )
		{
			const bool nan = std::isnan( p.temperatureInc ) || std::isnan( p.logprobThold ) || std::isnan( p.entropyThold ) || std::isnan( p.noSpeechThold );
			if( !nan && !( p.temperatureInc > 0.0f && p.temperatureInc < 0.01f ) ) return S_OK;
			logError( "%s: a threshold is NaN, or temperatureInc lies in ( 0, 0.01 )", name );
			return E_INVALIDARG;
		}
		inline HRESULT checkSuppressed( const char* name, const int32_t* ids, uint32_t count, int tokenEot )
		{
			if( count && !ids ) return E_POINTER;
			for( uint32_t i = 0; i < count; i++ )
				if( ids[ i ] < 0 || ids[ i ] >= tokenEot )
				{
					logError( "%s: id %i is outside [ 0, %i ): only text tokens can be suppressed", name, (int)ids[ i ], tokenEot );
					return E_INVALIDARG;
				}
			return S_OK;
		}
		// set: the checked copy of the caller's phrases, empty for nullptr
		inline HRESULT checkBoosted( const char* name, const sBoostedPhrases* p, int tokenEot, phraseBoost::Set& set )
		{
			set = phraseBoost::Set{};
			std::string text;
			const char* const why = p ? phraseBoost::check( p->tokens, p->lengths, p->count, p->maxLength, p->boost, tokenEot, set, text ) : nullptr;
			if( !why ) return S_OK;
			logError( "%s: %s", name, why );
			return E_INVALIDARG;
		}
		// n of the no-repeat n-gram rule: 0 = off, 1 .. 8 on (the compute layer's NRN_MAX_N)
		inline HRESULT checkNoRepeat( const char* name, int n )
		{
			if( n >= 0 && n <= 8 ) return S_OK;
			logError( "%s: n = %i is outside 0 .. 8", name, n );
			return E_INVALIDARG;
		}
		// the speech filter's parameters: frames, each 0 (the default) .. 2^20 (speechSpans.h states the defaults and the bound); flags reserved
		inline HRESULT checkSpeechFilter( const char* name, const sSpeechFilter& p )
		{
			int64_t a = p.minSilenceFrames, b = p.minSpeechFrames, c = p.padFrames;
			if( p.flags == 0 && SUCCEEDED( speechRules::resolveParams( a, b, c ) ) ) return S_OK;
			logError( "%s: minSilenceFrames, minSpeechFrames and padFrames must each lie in 0 .. 2^20 frames, and flags must be 0", name );
			return E_INVALIDARG;
		}
		// BatchRunner without the injected device entry an option needs (batchSampling.h and its like)
		inline HRESULT notGiven( const char* name, const char* what )
		{
			logError( "%s: this build of the scheduler was not given the device's %s", name, what );
			return E_NOTIMPL;
		}

		// A public function on the object behind its interface pointer: call( Impl& ) when the object is this library's. notOurs says what it is not
		// (the caller's one sentence for a foreign context or runner); hint, when given, says in brackets who takes the call instead ("a batch runner takes setBatch...").
		template<class Impl, class I, class Call>
		inline HRESULT forward( I* object, const char* name, const char* notOurs, const char* hint, Call&& call )
		{
			if( !object ) return E_POINTER;
			Impl* const impl = dynamic_cast<Impl*>( object );
			if( impl ) return call( *impl );
			if( hint ) logError( "%s: %s (%s)", name, notOurs, hint );
			else logError( "%s: %s", name, notOurs );
			return E_INVALIDARG;
		}
	}
}
