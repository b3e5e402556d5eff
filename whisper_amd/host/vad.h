// Voice-activity decision over precomputed features: the loop of VAD::detect restated (Whisper/Whisper/voiceActivityDetection.cpp:121-205; Moattar &
// Homayounpour 2009, section 3). Host only, no device, no other header of this library than the API's: tests/vad_cpu/driver.cpp compiles it alone.
//
// The per-frame features -- energy, dominant frequency F, spectral flatness SFM of 256-sample frames -- come from the device (wh_vad_features of
// whisper_hip.h: a DFT and 256 logarithms per frame); what is left is a few comparisons per frame that depend on the frame before, which is host work.
#pragma once
#include "whisperApi.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace Whisper
{
	namespace vad
	{
		constexpr int64_t FRAME_SAMPLES = 256;	   // FFT_POINTS: 16 ms at 16 kHz
		constexpr int64_t MIN_FRAMES = 30;		   // the feature minima are taken over the first 30 frames
		// primary thresholds (defaultPrimaryThresholds): the energy's is scaled by log10 of the running energy minimum
		constexpr float THR_ENERGY = 40.0f, THR_F = 185.0f, THR_SFM = 5.0f;

		// The loop's state between two frames, so that it can stop after any frame and go on later: VAD::State (voiceActivityDetection.h), which the capture loop
		// keeps across reads (detect continues at its frame i, :131-142, :196-202). feed() on any split of a feature array leaves the state, and returns the
		// lastSpeech, that one call on the whole array does: the arithmetic below is the only statement of the loop, decide() is feed() from a cleared state.
		struct Detector
		{
			float minEnergy = 0.0f, minF = 0.0f, minSfm = 0.0f, silenceRun = 0.0f;
			int64_t i = 0, lastSpeech = 0;

			void clear() { *this = Detector{}; }
			// feat: the features of frames i .. i + nFrames - 1; speech (may be nullptr): one byte per fed frame
			// Single precision exactly as the reference writes it; NaN and infinities go where C++ float comparisons send them: std::min( m, c ) is c only
			// when c < m, so a NaN minimum (an all-zero first frame has SFM 0 / 0) stays and a NaN feature never becomes one; `>=` with a NaN is false;
			// log10f( 0 ) = -inf makes the energy test true for every number.
			int64_t feed( const float* feat, int64_t nFrames, uint8_t* speech = nullptr )
			{
				for( int64_t k = 0; k < nFrames; k++, i++ )
				{
					const float energy = feat[ 3 * k ], F = feat[ 3 * k + 1 ], sfm = feat[ 3 * k + 2 ];
					if( i == 0 ) { minEnergy = energy; minF = F; minSfm = sfm; }
					else if( i < MIN_FRAMES )
					{
						minEnergy = std::min( minEnergy, energy );
						minF = std::min( minF, F );
						minSfm = std::min( minSfm, sfm );
					}
					const float thrEnergy = THR_ENERGY * std::log10( minEnergy );
					int votes = 0;
					if( ( energy - minEnergy ) >= thrEnergy ) votes++;
					if( ( F - minF ) >= THR_F ) votes++;
					if( ( sfm - minSfm ) >= THR_SFM ) votes++;
					const bool isSpeech = votes > 1;
					if( isSpeech )
					{
						lastSpeech = ( i + 1 ) * FRAME_SAMPLES;
						silenceRun = 0.0f;
					}
					else
					{
						// a silent frame pulls the energy minimum towards itself
						silenceRun += 1.0f;
						minEnergy = ( ( silenceRun * minEnergy ) + energy ) / ( silenceRun + 1.0f );
					}
					if( speech ) speech[ k ] = isSpeech ? 1 : 0;
				}
				return lastSpeech;
			}
		};

		// feat: [nFrames][3] = energy, F, SFM. speech (may be nullptr): one byte per frame, 1 = speech. Returns `lastSpeech`: ( i + 1 ) * 256 of the last
		// speech frame, 0 if there is none -- what the reference's detect returns for the whole buffer.
		inline int64_t decide( const float* feat, int64_t nFrames, uint8_t* speech )
		{
			Detector d;
			return d.feed( feat, nFrames, speech );
		}
	}
}
