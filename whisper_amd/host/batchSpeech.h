// Speech only in the lock-step batch runner ("Speech only"): the device half as the scheduler reaches it, the signature of
// wh_context_speech_filter. batchScheduler.cpp holds NO reference to that symbol -- its CPU test library links against a test double of the compute layer that
// does not have it: whisperImpl.cpp installs &wh_context_speech_filter here when libWhisper.so is loaded, a test library installs its own (a host copy).
// nullptr: turning the filter on in Whisper::setBatchSpeechFilter answers E_NOTIMPL.
#pragma once
#include "whisper_hip.h"

namespace Whisper
{
	using pfnBatchSpeechPacker = int ( * )( wh_context* c, const float* pcmDev, int64_t nSamples, const float* stereoDev, const wh_speech_params* params,
		const float** packedDev, const float** packedStereoDev, int64_t* nPacked, int64_t* spansOut, int cap, int* count );
	extern pfnBatchSpeechPacker g_batchSpeechPacker;
}
