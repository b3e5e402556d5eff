// Where to cut a long recording into the independent pieces of at most 30 s that the lock-step batch runner takes (sBatchStream::firstSample /
// countSamples): at pauses found by the voice-activity decision (vad.h), so that no word straddles a boundary. The reference uses the same detector to
// fire a transcription when the speaker pauses (Whisper/Whisper/ContextImpl.capture.cpp, pauseDuration = 0.333 s); used to choose chunk boundaries it
// puts ONE long recording on the batched path. Host only, no device: tests/vad_cpu/driver.cpp compiles it alone.
//
//   start = 0
//   while N - start > maxLen:
//       hi = floor( min( start + maxLen, N - 16000 ) / 256 )       a tail under one second would come back empty (runFull's S_FALSE)
//       lo = ceil( ( start + minLen ) / 256 )
//       for every pause [a, b) in order: c = min( ( a + b ) div 2, hi ); if lo <= c and a < c < b: cut = c         the last one wins: the longest chunk
//       no such pause: cut = the first c in [lo, hi] with c >= 10 and c + 11 <= nFrames that minimises sum energy[ c - 10 .. c + 10 ] (summed in double)
//       emit ( start, 256 cut - start ); start = 256 cut
//   emit ( start, N - start )
// A pause is a maximal run [a, b) of at least pauseFrames non-speech frames. By construction the plan is a partition of [0, N); every chunk but the last
// starts and ends on a multiple of 256; no chunk is longer than maxLen; every chunk but the last is at least minLen, and the last at least 16000 whenever
// N >= 16000; N <= maxLen gives one chunk. It is a function of the samples alone: every rank of whisper-mgpu computes the same plan.
#pragma once
#include "whisperApi.h"
#include "vad.h"
#include <cstdint>
#include <limits>
#include <utility>
#include <vector>

namespace Whisper
{
	namespace chunkPlanner
	{
		constexpr int64_t MAX_LEN = 480000, MIN_LEN = 240000, PAUSE_FRAMES = 21;	 // 30 s, 15 s, 0.336 s: the first whole frame count >= the reference's 0.333 s
		constexpr int64_t MIN_TAIL = 16000;		   // shorter recordings are not transcribed
		constexpr int64_t ENERGY_HALF = 10;		   // the fallback looks at 21 frames = 0.336 s around a candidate

		struct Chunk { int64_t firstSample, countSamples; };

		// 0 = the default of each parameter
		inline HRESULT resolveParams( int64_t& maxLen, int64_t& minLen, int64_t& pauseFrames )
		{
			if( maxLen == 0 ) maxLen = MAX_LEN;
			if( minLen == 0 ) minLen = MIN_LEN;
			if( pauseFrames == 0 ) pauseFrames = PAUSE_FRAMES;
			if( maxLen > MAX_LEN || minLen < MIN_TAIL || minLen > maxLen - 2 * MIN_TAIL || pauseFrames < 1 ) return E_INVALIDARG;
			return S_OK;
		}

		// speech: one byte per frame (vad::decide), energy: the frames' energies, nFrames = N / 256 of the recording's N samples
		inline HRESULT plan( const uint8_t* speech, const float* energy, int64_t nFrames, int64_t N, int64_t maxLen, int64_t minLen, int64_t pauseFrames,
			std::vector<Chunk>& chunks )
		{
			chunks.clear();
			const HRESULT hr = resolveParams( maxLen, minLen, pauseFrames );
			if( FAILED( hr ) ) return hr;
			if( N < 0 || nFrames != N / vad::FRAME_SAMPLES || ( nFrames > 0 && ( !speech || !energy ) ) ) return E_INVALIDARG;

			std::vector<std::pair<int64_t, int64_t>> pauses;
			for( int64_t i = 0; i < nFrames; )
			{
				if( speech[ i ] ) { i++; continue; }
				int64_t b = i;
				while( b < nFrames && !speech[ b ] ) b++;
				if( b - i >= pauseFrames ) pauses.emplace_back( i, b );
				i = b;
			}

			int64_t start = 0;
			while( N - start > maxLen )
			{
				const int64_t hi = std::min( start + maxLen, N - MIN_TAIL ) / vad::FRAME_SAMPLES;
				const int64_t lo = ( start + minLen + vad::FRAME_SAMPLES - 1 ) / vad::FRAME_SAMPLES;
				int64_t cut = -1;
				for( const auto& p : pauses )
				{
					const int64_t c = std::min( ( p.first + p.second ) / 2, hi );
					if( lo <= c && p.first < c && c < p.second ) cut = c;
				}
				if( cut < 0 )
				{
					double best = std::numeric_limits<double>::infinity();
					for( int64_t c = lo; c <= hi; c++ )
					{
						if( c < ENERGY_HALF || c + ENERGY_HALF + 1 > nFrames ) continue;
						double sum = 0.0;
						for( int64_t k = c - ENERGY_HALF; k <= c + ENERGY_HALF; k++ ) sum += (double)energy[ k ];
						if( sum < best ) { best = sum; cut = c; }
					}
					// energies that are all NaN or +inf (samples that are): the longest chunk
					if( cut < 0 ) cut = hi;
				}
				chunks.push_back( Chunk{ start, vad::FRAME_SAMPLES * cut - start } );
				start = vad::FRAME_SAMPLES * cut;
			}
			chunks.push_back( Chunk{ start, N - start } );
			return S_OK;
		}
	}
}
