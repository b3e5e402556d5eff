// Stereo diarization, iContext::detectSpeaker: which channel of a stereo recording is louder during a segment. The reference's rule restated
// (Whisper/Whisper/ContextImpl.diarize.cpp:9-108 with Spectrogram::copyStereoPcm, Spectrogram.cpp:142-168). Host only, no device, no other header of
// this library than the API's: tests/diarize_cpu/driver.cpp compiles it alone.
//
// No kernel: a segment is a few hundred thousand additions (a whole 200 s clip 6.4 M), microseconds on one host core and once per segment, over PCM
// that is on the host already because iAudioBuffer::getPcmStereo() has to return it. Uploading it to add it up would cost more than the sum.
#pragma once
#include "whisperApi.h"
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifndef OLE_E_BLANK
#define OLE_E_BLANK ( (HRESULT)0x80040007 )
#endif

namespace Whisper
{
	namespace diarize
	{
		constexpr int64_t CHUNK_SAMPLES = 160;	   // FFT_STEP: the 10 ms chunks segment times are counted in

		// A timestamp in 100 ns ticks -> 10 ms chunks from the start of the buffer; C++ division, which truncates towards zero (diarize.cpp:9-13)
		inline int64_t chunkOffset( int64_t ticks, int64_t mediaTimeOffset )
		{
			ticks -= mediaTimeOffset;
			return ( ticks * 100 ) / 10'000'000;
		}

		// Sum of |sample| per channel over `frames` interleaved stereo frames, in the reference's order (diarize.cpp:35-51): its SSE accumulator holds
		// ( left, right ) of the even frames in lanes 0-1 and of the odd frames in lanes 2-3, every lane added to sequentially; a trailing odd frame is
		// loaded into lanes 0-1 -- its index is even, so one loop over i & 1 says the same. Then lanes 0 + 2 and 1 + 3. Single precision throughout: a
		// comparison near the threshold must come out as the reference's does.
		inline void channelsEnergy( const float* stereo, size_t frames, float& left, float& right )
		{
			float acc[ 4 ] = { 0.0f, 0.0f, 0.0f, 0.0f };
			for( size_t i = 0; i < frames; i++ )
			{
				float* const a = acc + ( i & 1 ) * 2;
				a[ 0 ] += std::fabs( stereo[ 2 * i ] );
				a[ 1 ] += std::fabs( stereo[ 2 * i + 1 ] );
			}
			left = acc[ 0 ] + acc[ 2 ];
			right = acc[ 1 ] + acc[ 3 ];
		}

		// `if( energy0 > 1.1 * energy1 ) speaker 0; else if( energy1 > 1.1 * energy0 ) speaker 1; else speaker ?` with the products in single
		// precision (diarize.cpp:54-70). A NaN compares false both ways: Unsure.
		inline eSpeakerChannel verdict( float left, float right )
		{
			if( left > 1.1f * right ) return eSpeakerChannel::Left;
			if( right > 1.1f * left ) return eSpeakerChannel::Right;
			return eSpeakerChannel::Unsure;
		}

		// ContextImpl::detectSpeaker once a run's audio is current. stereo: the run's interleaved 16 kHz stereo PCM, `frames` frames of it (nullptr / 0:
		// the audio was loaded without stereo data). The slice starts at chunk `begin` and is `len` chunks long; frames past the end of the buffer count
		// as zero (adding +0 changes no accumulator, so they are not visited); a start at or past the end is E_BOUNDS, and so is a negative `begin`,
		// which the reference's cast to size_t sends to the same branch. Times more than 2^63 / 100 ticks (29 000 years) from the offset overflow, as
		// they do in the reference.
		inline HRESULT detectSpeaker( const float* stereo, size_t frames, int64_t mediaTimeOffset, const sTimeInterval& time, eSpeakerChannel& result )
		{
			const int64_t begin = chunkOffset( (int64_t)time.begin.ticks, mediaTimeOffset );
			const int64_t end = chunkOffset( (int64_t)time.end.ticks, mediaTimeOffset );
			const int64_t len = end - begin;
			if( len <= 0 )
			{
				result = eSpeakerChannel::Unsure;
				return S_OK;
			}
			if( !stereo || frames == 0 )
			{
				result = eSpeakerChannel::NoStereoData;
				return S_OK;
			}
			// begin * 160 >= frames, without the product
			const uint64_t chunks = ( (uint64_t)frames + CHUNK_SAMPLES - 1 ) / CHUNK_SAMPLES;
			if( begin < 0 || (uint64_t)begin >= chunks ) return E_BOUNDS;
			const size_t first = (size_t)begin * CHUNK_SAMPLES, rest = frames - first;
			const size_t count = (uint64_t)len >= chunks ? rest : ( (size_t)len * CHUNK_SAMPLES < rest ? (size_t)len * CHUNK_SAMPLES : rest );
			float left, right;
			channelsEnergy( stereo + 2 * first, count, left, right );
			result = verdict( left, right );
			return S_OK;
		}
	}
}
