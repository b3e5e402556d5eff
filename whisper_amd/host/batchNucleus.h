// Top-k and nucleus sampling in the lock-step batch runner ("Top-k and nucleus sampling"): the device half as the scheduler reaches it, the
// signature of wh_context_set_nucleus. batchScheduler.cpp holds NO reference to that symbol -- its CPU test library links against a test double of the compute
// layer that does not have it: whisperImpl.cpp installs &wh_context_set_nucleus here when libWhisper.so is loaded, a test library installs its own. nullptr:
// turning the filter on in Whisper::setBatchSamplingFilter answers E_NOTIMPL.
#pragma once
#include "whisper_hip.h"

namespace Whisper
{
	using pfnBatchNucleus = int ( * )( wh_context* c, int topK, float topP );
	extern pfnBatchNucleus g_batchNucleus;
}
