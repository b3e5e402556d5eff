// Decoding fallback in the lock-step batch runner ("The batch runner"): the device half as the scheduler reaches it. A round's slots stand
// at different attempts of their windows' FallbackPlans (decodeFallback.h), so the device needs a temperature, a Philox key and a nonce PER ROW
// (wh_context_set_sampling_rows), and the no-speech gather of the prompt step (wh_context_set_no_speech / wh_decode_window_no_speech). batchScheduler.cpp holds
// NO reference to those symbols -- its CPU test library links against a test double of the compute layer that does not have them: whisperImpl.cpp installs
// the table below when libWhisper.so is loaded, a test library installs its own. nullptr: Whisper::setBatchDecodingFallback answers E_NOTIMPL.
#pragma once
#include "whisper_hip.h"
#include <cstdint>

namespace Whisper
{
	struct BatchSamplingHooks
	{
		// rows HOST arrays: row r greedy at temperature 0, else sampled at temperature[ r ] under seed[ r ] and nonce[ r ]; rows == 0 turns the mode off
		int ( *setRowSampling )( wh_context* c, int rows, const float* temperature, const uint64_t* seed, const uint32_t* nonce );
		// on: the next window starts gather P( <|nospeech|> ) of every row's prompt step
		int ( *setNoSpeech )( wh_context* c, int on );
		// HOST float per row of the window in progress
		int ( *readNoSpeech )( wh_context* c, float* out );
	};
	extern const BatchSamplingHooks* g_batchSamplingHooks;
}
