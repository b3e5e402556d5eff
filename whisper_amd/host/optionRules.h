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
		// top-k and nucleus sampling: topK 0 (off) .. 1024 (the compute layer's NUCLEUS_MAX_K), topP in ( 0, 1 ], 1 = off
		inline HRESULT checkSamplingFilter( const char* name, int topK, float topP )
		{
			if( topK >= 0 && topK <= 1024 && topP > 0.0f && topP <= 1.0f ) return S_OK;
			logError( "%s: topK = %i is outside 0 .. 1024, or topP = %g is outside ( 0, 1 ]", name, topK, (double)topP );
			return E_INVALIDARG;
		}
		// constrained decoding: the automaton's limits (the compute layer's CON_MAX_*), every transition in [ -1, states ), every class below `classes`, the penalty
		inline HRESULT checkConstraint( const char* name, const sDecodingConstraint* p )
		{
			if( !p ) return S_OK;
			if( !p->classOf || !p->transitions || !p->accept ) return E_POINTER;
			const auto refuse = [ & ]( const char* why, long long v ) { logError( "%s: %s (%lli)", name, why, v ); return E_INVALIDARG; };
			if( p->states < 1 || p->states > 4096 ) return refuse( "a constraint has 1 .. 4096 states", (long long)p->states );
			if( p->classes < 1 || p->classes > 256 ) return refuse( "a constraint has 1 .. 256 byte classes", (long long)p->classes );
			if( (uint64_t)p->states * p->classes > 65536 ) return refuse( "states * classes is above 65536, the transition table of one constraint", (long long)p->states * p->classes );
			if( p->start >= p->states ) return refuse( "the start state is outside [ 0, states )", (long long)p->start );
			if( !( p->penalty > 0.0f ) ) return refuse( "the penalty must be greater than 0 (+inf is allowed, NaN is not)", 0 );
			for( int i = 0; i < 256; i++ )
				if( p->classOf[ i ] >= p->classes ) return refuse( "a byte's class is outside [ 0, classes ), byte", i );
			for( uint32_t i = 0; i < p->states * p->classes; i++ )
				if( p->transitions[ i ] < -1 || p->transitions[ i ] >= (int32_t)p->states ) return refuse( "a transition is outside [ -1, states ), entry", (long long)i );
			return S_OK;
		}
		// the speech filter's parameters: frames, each 0 (the default) .. 2^20 (speechSpans.h states the defaults and the bound); flags reserved
		inline HRESULT checkSpeechFilter( const char* name, const sSpeechFilter& p )
		{
			int64_t a = p.minSilenceFrames, b = p.minSpeechFrames, c = p.padFrames;
			if( p.flags == 0 && SUCCEEDED( speechRules::resolveParams( a, b, c ) ) ) return S_OK;
			logError( "%s: minSilenceFrames, minSpeechFrames and padFrames must each lie in 0 .. 2^20 frames, and flags must be 0", name );
			return E_INVALIDARG;
		}
		// What a lock-step batch does not decode, whatever its caches: beam search and AlignTokens are iContext::runFull's. A runner with FP8 cross-attention caches
		// (sBatchSetup::flags bit 2) could serve neither -- the hypothesis-group kernel and the alignment kernels read FP16 rows -- and answers the same E_NOTIMPL.
		inline HRESULT checkBatchDecoding( const char* name, bool beam, bool align )
		{
			if( beam ) logError( "%s: eSamplingStrategy::BeamSearch is not available in a lock-step batch; use iContext::runFull", name );
			else if( align ) logError( "%s: eFullParamsFlags::AlignTokens is not available in a lock-step batch; use iContext::runFull", name );
			return beam || align ? E_NOTIMPL : S_OK;
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
