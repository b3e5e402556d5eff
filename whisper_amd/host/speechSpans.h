// Which samples of a recording are speech, and where a time on the packed copy of them lies in the recording: the rules behind Whisper::setSpeechFilter
// (transcribe the speech only, report times on the original clock -- what faster-whisper calls vad_filter and whisper.cpp --vad). Host only, no device, no
// other header of this library than the API's and vad.h: tests/speech_spans_cpu/driver.cpp compiles it alone.
//
// Input: the speech flags of vad::decide (one byte per 256-sample frame) and the recording's N samples. Parameters in frames, 0 = the default:
// minSilenceFrames 125 (2.0 s), minSpeechFrames 16 (0.256 s), padFrames 25 (0.4 s) -- faster-whisper's vad_filter values rounded to frames; nobody has measured
// them for this detector on real speech. The detector's flags are choppy (hundreds of runs under 16 frames on an ordinary recording), so runs are merged BEFORE
// short ones are dropped:
//   1. the maximal runs of speech frames
//   2. neighbours separated by fewer than minSilenceFrames non-speech frames become one run
//   3. merged runs shorter than minSpeechFrames are dropped
//   4. every run grows by padFrames on both sides, clamped to [0, nFrames]; runs that now touch or overlap become one
//   5. a run that ends at nFrames also takes the recording's last partial frame: it ends at N
// The spans are sample ranges [a, b), ascending and disjoint; every a is a multiple of 256, every b too except that the last may be N.
//
// The time map works in samples; out[i] is the position of span i in the packed copy (out[0] = 0, out[count] = the packed length).
//   start rule   packed s -> a_i + ( s - out[i] ) for the span with out[i] <= s < out[i + 1]; s = the packed length -> the last span's end, and a position
//                behind the packed copy (the decoder may name a time behind its audio) lies as far behind the last span's end
//   end rule     s > 0 -> ( the start rule of s - 1 ) + 1, so that a range that ends exactly at a join ends where the earlier span ends; s = 0 -> a_0
// Both are non-decreasing, and the identity when one span covers [0, N). Times enter and leave as 100 ns ticks, a sample is 625 of them: a start time
// keeps its ticks past the sample it lies in, an end time its ticks short of the sample boundary it lies at or before.
#pragma once
#include "whisperApi.h"
#include "vad.h"
#include <algorithm>
#include <cstdint>
#include <vector>

namespace Whisper
{
	namespace speechRules
	{
		constexpr int64_t MIN_SILENCE_FRAMES = 125, MIN_SPEECH_FRAMES = 16, PAD_FRAMES = 25;
		constexpr int64_t MAX_PARAM_FRAMES = (int64_t)1 << 20;
		constexpr int64_t TICKS_PER_SAMPLE = 625;	  // 100 ns ticks at 16 kHz

		struct Span { int64_t a, b; };

		// 0 = the default of each parameter
		inline HRESULT resolveParams( int64_t& minSilenceFrames, int64_t& minSpeechFrames, int64_t& padFrames )
		{
			for( const int64_t v : { minSilenceFrames, minSpeechFrames, padFrames } )
				if( v < 0 || v > MAX_PARAM_FRAMES ) return E_INVALIDARG;
			if( minSilenceFrames == 0 ) minSilenceFrames = MIN_SILENCE_FRAMES;
			if( minSpeechFrames == 0 ) minSpeechFrames = MIN_SPEECH_FRAMES;
			if( padFrames == 0 ) padFrames = PAD_FRAMES;
			return S_OK;
		}

		// speech: one byte per frame (vad::decide), nFrames = N / 256 of the recording's N samples
		inline HRESULT find( const uint8_t* speech, int64_t nFrames, int64_t N, int64_t minSilenceFrames, int64_t minSpeechFrames, int64_t padFrames,
			std::vector<Span>& spans )
		{
			spans.clear();
			const HRESULT hr = resolveParams( minSilenceFrames, minSpeechFrames, padFrames );
			if( FAILED( hr ) ) return hr;
			if( N < 0 || nFrames != N / vad::FRAME_SAMPLES || ( nFrames > 0 && !speech ) ) return E_INVALIDARG;

			// rules 1 and 2, in frames: a run joins the one before it when the gap between them is short
			std::vector<Span> runs;
			for( int64_t i = 0; i < nFrames; )
			{
				if( !speech[ i ] ) { i++; continue; }
				int64_t e = i;
				while( e < nFrames && speech[ e ] ) e++;
				if( !runs.empty() && i - runs.back().b < minSilenceFrames ) runs.back().b = e;
				else runs.push_back( Span{ i, e } );
				i = e;
			}
			// rules 3 and 4
			std::vector<Span> wide;
			for( const Span& r : runs )
			{
				if( r.b - r.a < minSpeechFrames ) continue;
				const int64_t a = std::max<int64_t>( r.a - padFrames, 0 ), b = std::min( r.b + padFrames, nFrames );
				if( !wide.empty() && a <= wide.back().b ) wide.back().b = std::max( wide.back().b, b );
				else wide.push_back( Span{ a, b } );
			}
			// rule 5, and frames become samples
			for( const Span& r : wide )
				spans.push_back( Span{ r.a * vad::FRAME_SAMPLES, r.b == nFrames ? N : r.b * vad::FRAME_SAMPLES } );
			return S_OK;
		}

		inline int64_t packedLength( const std::vector<Span>& spans )
		{
			int64_t n = 0;
			for( const Span& s : spans ) n += s.b - s.a;
			return n;
		}
		// one span that is the whole recording: the packed copy is the recording
		inline bool coversAll( const std::vector<Span>& spans, int64_t N ) { return spans.size() == 1 && spans[ 0 ].a == 0 && spans[ 0 ].b == N; }

		class TimeMap
		{
			std::vector<Span> spans;
			std::vector<int64_t> out;	// count + 1 packed positions
		public:
			TimeMap() = default;
			explicit TimeMap( const std::vector<Span>& s ) { assign( s ); }
			void assign( const std::vector<Span>& s )
			{
				spans = s;
				out.assign( s.size() + 1, 0 );
				for( size_t i = 0; i < s.size(); i++ ) out[ i + 1 ] = out[ i ] + ( s[ i ].b - s[ i ].a );
			}
			bool empty() const { return spans.empty(); }
			int64_t packedLength() const { return out.empty() ? 0 : out.back(); }
			const std::vector<Span>& all() const { return spans; }

			// packed sample position -> sample position of the recording; a negative position counts as 0. No span: the identity.
			int64_t start( int64_t s ) const
			{
				if( spans.empty() ) return s;
				if( s >= out.back() ) return spans.back().b + ( s - out.back() );
				if( s < 0 ) s = 0;
				// the span with out[i] <= s < out[i + 1]: the last i whose out[i] <= s
				const size_t i = (size_t)( std::upper_bound( out.begin(), out.end() - 1, s ) - out.begin() ) - 1;
				return spans[ i ].a + ( s - out[ i ] );
			}
			int64_t end( int64_t s ) const
			{
				if( spans.empty() ) return s;
				if( s <= 0 ) return spans.front().a;
				return start( s - 1 ) + 1;
			}
			// the same in 100 ns ticks
			int64_t startTicks( int64_t t ) const
			{
				if( t < 0 ) t = 0;
				const int64_t s = t / TICKS_PER_SAMPLE;
				return start( s ) * TICKS_PER_SAMPLE + ( t - s * TICKS_PER_SAMPLE );
			}
			int64_t endTicks( int64_t t ) const
			{
				if( t < 0 ) t = 0;
				const int64_t s = ( t + TICKS_PER_SAMPLE - 1 ) / TICKS_PER_SAMPLE;
				if( s == 0 ) return end( 0 ) * TICKS_PER_SAMPLE;
				return end( s ) * TICKS_PER_SAMPLE - ( s * TICKS_PER_SAMPLE - t );
			}
		};
	}
}
