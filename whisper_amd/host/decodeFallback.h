// Decoding fallback: the host rules. A window's attempt is scored, and the plan says what happens next: accept it, decode the window again
// at the next temperature, skip the window as silence, or hand the last attempt over as it stands. As openai-whisper (transcribe.py, decode_with_fallback) and
// whisper.cpp do it; the reference has nothing of the kind. Host only, no device, no other header of this library than the API's: tests/fallback_cpu/driver.cpp
// compiles it alone. The device half -- the tempered softmax, the draw, the no-speech probability -- is behind wh_context_set_sampling / _set_no_speech.
#pragma once
#include "whisperApi.h"
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <map>
#include <vector>

namespace Whisper
{
	namespace fallback
	{
		constexpr int ENTROPY_TOKENS = 32;	   // the entropy looks at the last 32 tokens; shorter attempts are not judged by it

		// 0, inc, 2 inc, ... while <= 1.0 + 1e-6, each k * inc formed in float. inc <= 0 (or NaN): the greedy attempt only.
		inline std::vector<float> schedule( float inc )
		{
			std::vector<float> t{ 0.0f };
			if( !( inc > 0.0f ) ) return t;
			for( int k = 1;; k++ )
			{
				const float v = (float)k * inc;
				if( !( (double)v <= 1.0 + 1e-6 ) ) break;
				t.push_back( v );
			}
			return t;
		}

		struct Scores
		{
			double avgLogprob = 0.0, entropy = 0.0;
		};
		// Over tokens[ 0 .. resultLen ), timestamps included. Token: anything with an integer `id` and a float `p`.
		//   avgLogprob = sum ln( max( p, FLT_MIN ) ) / resultLen, added in token order in double (a NaN p counts as FLT_MIN); 0 for an empty attempt
		//   entropy    = - sum_v q_v ln q_v over the distinct ids v of the last min( 32, resultLen ) tokens in ascending id order, q_v = count / n
		template<class Token>
		inline Scores score( const Token* tokens, int resultLen )
		{
			Scores s;
			if( resultLen <= 0 ) return s;
			double sum = 0.0;
			for( int i = 0; i < resultLen; i++ )
			{
				const float p = tokens[ i ].p;
				sum += std::log( (double)( p > FLT_MIN ? p : FLT_MIN ) );
			}
			s.avgLogprob = sum / (double)resultLen;
			const int n = resultLen < ENTROPY_TOKENS ? resultLen : ENTROPY_TOKENS;
			std::map<int, int> counts;
			for( int i = resultLen - n; i < resultLen; i++ ) counts[ (int)tokens[ i ].id ]++;
			double h = 0.0;
			for( const auto& kv : counts )
			{
				const double q = (double)kv.second / (double)n;
				h -= q * std::log( q );
			}
			s.entropy = h;
			return s;
		}

		// What the gates see of one attempt
		struct Attempt
		{
			bool scanFailed = false;   // WindowScan::failed
			int resultLen = 0;
			Scores scores;
			float noSpeech = 0.0f;	   // P( <|nospeech|> ) of the window's prompt step
		};
		inline bool attemptFailed( const sDecodingFallback& f, const Attempt& a )
		{
			return a.scanFailed || a.resultLen == 0 || a.scores.avgLogprob < (double)f.logprobThold ||
				( a.resultLen > ENTROPY_TOKENS && a.scores.entropy < (double)f.entropyThold );
		}
		// silence wins: a window the model itself calls silent is dropped however it was scored, unless the stop rules failed it (their own retry-or-skip applies)
		inline bool attemptSilent( const sDecodingFallback& f, const Attempt& a )
		{
			return !a.scanFailed && a.noSpeech > f.noSpeechThold && a.scores.avgLogprob < (double)f.logprobThold;
		}

		enum struct eVerdict : int
		{
			Accept = 0,		// the attempt passed: hand it to finishWindow
			Retry = 1,		// it failed: decode the window again at temperature()
			Skip = 2,		// silence: hand finishWindow a scan without tokens
			HandOver = 3,	// it failed and no temperature is left: hand it to finishWindow as it stands
		};

		// The sequence of attempts of ONE window
		class FallbackPlan
		{
			const sDecodingFallback params;
			const std::vector<float> temps;
			const int seek;
			int index = 0;

		public:
			FallbackPlan( const sDecodingFallback& p, int windowSeek ) : params( p ), temps( schedule( p.temperatureInc ) ), seek( windowSeek ) {}
			// of the attempt to decode now
			float temperature() const { return temps[ (size_t)index ]; }
			int attemptIndex() const { return index; }
			int attempts() const { return index + 1; }
			uint64_t seed() const { return params.seed; }
			// distinct for the attempts of a window and the windows of a stream (windows lie at least 100 frames apart)
			uint32_t nonce() const { return (uint32_t)seek * 8u + (uint32_t)index; }
			// the attempt just decoded; Retry moves the plan to the next temperature
			eVerdict judge( const Attempt& a )
			{
				if( attemptSilent( params, a ) ) return eVerdict::Skip;
				if( !attemptFailed( params, a ) ) return eVerdict::Accept;
				if( (size_t)index + 1 < temps.size() )
				{
					index++;
					return eVerdict::Retry;
				}
				return eVerdict::HandOver;
			}
		};
	}
}
