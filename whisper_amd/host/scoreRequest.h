// Scoring a given transcript (Whisper::scoreTokens / scoreBatch, include/whisperApi.h): the rules of a request, stated once. Header only, no device calls --
// scoreTranscripts.cpp and the lock-step scheduler's scorer share it, and tests/score_cpu/driver.cpp compiles it into a stand-alone program.
//   * the row a request becomes: prompt + tokens + eot, scored from the first token behind the prompt;
//   * every argument check: the clip, ids inside the vocabulary, the length against the bound of wh_score_tokens, an empty prompt or token list, the form
//     forced alignment needs;
//   * packing requests into the slots of lock-step passes and mapping the records of a pass back to the requests, in request order.
#pragma once
#include "whisperApi.h"
#include "whisper_hip.h"
#include <algorithm>
#include <vector>

namespace Whisper
{
	// The device half as the lock-step scheduler reaches it: the signature of wh_score_tokens. batchScheduler.cpp holds NO reference to that symbol (its CPU test
	// library links against a test double of the compute layer that does not have it): whisperImpl.cpp installs &wh_score_tokens here when libWhisper.so is
	// loaded, a test library installs its own. nullptr: Whisper::scoreBatch is E_NOTIMPL.
	using pfnBatchScorer = int ( * )( wh_context* c, int batch, const int32_t* tokens, const int32_t* lens, const int32_t* firstScored, int nMax, wh_token_score* outHost );
	extern pfnBatchScorer g_batchScorer;

	namespace score
	{
		constexpr uint32_t FLAG_ALIGN = 1;
		constexpr int64_t SAMPLE_RATE = 16000, CLIP_MIN = SAMPLE_RATE, CLIP_MAX = 30 * SAMPLE_RATE;	  // a clip of 1 to 30 s: one window
		constexpr int MAX_ROW = 256;	   // wh_score_tokens: nMax <= min( 256, n_text_ctx )

		// what the checks need of a model
		struct Limits
		{
			int nVocab, tokenEot, tokenNot, nTextCtx;
			int maxRow() const { return std::min( MAX_ROW, nTextCtx ); }
		};

		// The clip of a request inside a buffer of bufferSamples samples: countSamples 0 = to the end. E_INVALIDARG for a clip that leaves the buffer, is shorter
		// than a second or longer than 30 s (long-form scoring is out of scope).
		inline HRESULT clipRange( int64_t bufferSamples, int64_t firstSample, int64_t countSamples, int64_t& count )
		{
			if( firstSample < 0 || countSamples < 0 || firstSample > bufferSamples ) return E_INVALIDARG;
			count = countSamples == 0 ? bufferSamples - firstSample : countSamples;
			if( count > bufferSamples - firstSample ) return E_INVALIDARG;
			if( count < CLIP_MIN || count > CLIP_MAX ) return E_INVALIDARG;
			return S_OK;
		}

		// A request as the compute layer takes it: row b of wh_score_tokens
		struct Row
		{
			std::vector<int32_t> tokens;	 // prompt + scored tokens + eot
			int32_t firstScored = 0;		 // = promptCount
			bool align = false;
			uint32_t records() const { return (uint32_t)tokens.size() - (uint32_t)firstScored; }	  // count + 1: eot is scored too
		};

		inline HRESULT buildRow( const Limits& lim, const whisper_token* prompt, uint32_t promptCount, const whisper_token* tokens, uint32_t count, uint32_t flags, Row& row )
		{
			if( !prompt || !tokens ) return E_POINTER;
			if( promptCount == 0 || count == 0 ) return E_INVALIDARG;
			if( flags & ~FLAG_ALIGN ) return E_INVALIDARG;
			if( (uint64_t)promptCount + count + 1 > (uint64_t)lim.maxRow() ) return E_INVALIDARG;
			for( uint32_t i = 0; i < promptCount; i++ )
				if( prompt[ i ] < 0 || prompt[ i ] >= lim.nVocab ) return E_INVALIDARG;
			for( uint32_t i = 0; i < count; i++ )
				if( tokens[ i ] < 0 || tokens[ i ] >= lim.nVocab ) return E_INVALIDARG;
			row.align = 0 != ( flags & FLAG_ALIGN );
			if( row.align )
			{
				// wh_align_tokens takes [sot sequence, no-timestamps, text..., eot]: the no-timestamps token exactly once, as the prompt's last entry behind at least
				// one other token, and text tokens only
				if( promptCount < 2 || prompt[ promptCount - 1 ] != lim.tokenNot ) return E_INVALIDARG;
				if( std::count( prompt, prompt + promptCount, (whisper_token)lim.tokenNot ) != 1 ) return E_INVALIDARG;
				for( uint32_t i = 0; i < count; i++ )
					if( tokens[ i ] >= lim.tokenEot ) return E_INVALIDARG;
			}
			row.tokens.assign( prompt, prompt + promptCount );
			row.tokens.insert( row.tokens.end(), tokens, tokens + count );
			row.tokens.push_back( lim.tokenEot );
			row.firstScored = (int32_t)promptCount;
			return S_OK;
		}

		// Lock-step passes: the requests that passed their checks, in request order, up to maxSlots per pass. passes[ p ][ slot ] = the request's index.
		inline std::vector<std::vector<uint32_t>> packPasses( const std::vector<HRESULT>& status, uint32_t maxSlots )
		{
			std::vector<std::vector<uint32_t>> passes;
			if( maxSlots == 0 ) maxSlots = 1;
			for( uint32_t r = 0; r < (uint32_t)status.size(); r++ )
			{
				if( FAILED( status[ r ] ) ) continue;
				if( passes.empty() || passes.back().size() >= maxSlots ) passes.emplace_back();
				passes.back().push_back( r );
			}
			return passes;
		}

		// The arguments of one wh_score_tokens call for a pass: tokens [slots][nMax] (zero padding), lens, firstScored
		struct PassArgs
		{
			int nMax = 0;
			std::vector<int32_t> tokens, lens, first;
		};
		inline PassArgs packTokens( const std::vector<uint32_t>& pass, const std::vector<Row>& rows )
		{
			PassArgs a;
			for( uint32_t r : pass ) a.nMax = std::max( a.nMax, (int)rows[ r ].tokens.size() );
			a.tokens.assign( pass.size() * (size_t)a.nMax, 0 );
			for( size_t s = 0; s < pass.size(); s++ )
			{
				const Row& row = rows[ pass[ s ] ];
				std::copy( row.tokens.begin(), row.tokens.end(), a.tokens.begin() + (ptrdiff_t)( s * (size_t)a.nMax ) );
				a.lens.push_back( (int32_t)row.tokens.size() );
				a.first.push_back( row.firstScored );
			}
			return a;
		}
		// The records [slots][nMax] of a pass back to the requests: scores[ r ][ k ] = the record of the request's k-th scored token, time zero
		inline void unpackRecords( const std::vector<uint32_t>& pass, const std::vector<Row>& rows, const PassArgs& a, const wh_token_score* recs, sTokenScore* const* scores )
		{
			for( size_t s = 0; s < pass.size(); s++ )
			{
				const Row& row = rows[ pass[ s ] ];
				for( uint32_t k = 0; k < row.records(); k++ )
				{
					const wh_token_score& g = recs[ s * (size_t)a.nMax + (size_t)row.firstScored + k ];
					sTokenScore& o = scores[ pass[ s ] ][ k ];
					o.logprob = g.logprob; o.bestLogprob = g.bestLogprob; o.best = g.best; o.rank = g.rank;
					o.time.begin.ticks = o.time.end.ticks = 0;
				}
			}
		}

		// Forced alignment: frames = wh_align_tokens' row of a request (for each text token and then the end of the text the first 20 ms position it aligns to).
		// The frame-to-time rule of eFullParamsFlags::AlignTokens at seek 0 (hostLoop.h): a text token lasts from its frame to the next one's, in 10 ms units
		// t = 2 * frame; eot, a special token, gets the end of the token before it. offsetTicks = the clip's place in its buffer plus the buffer's media time.
		inline void alignedTimes( const int32_t* frames, uint32_t count, int64_t offsetTicks, sTokenScore* scores )
		{
			auto ticks = [ & ]( int32_t frame ) { return (uint64_t)( (int64_t)2 * frame * 100000 + offsetTicks ); };
			for( uint32_t k = 0; k < count; k++ )
			{
				scores[ k ].time.begin.ticks = ticks( frames[ k ] );
				scores[ k ].time.end.ticks = ticks( frames[ k + 1 ] );
			}
			scores[ count ].time.begin.ticks = scores[ count ].time.end.ticks = ticks( frames[ count ] );
		}
	}
}
