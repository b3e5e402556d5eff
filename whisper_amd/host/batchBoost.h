// Phrase boosting in the lock-step batch runner ("Phrase boosting"): the device half as the scheduler reaches it, the signature of
// wh_context_set_boost. batchScheduler.cpp holds NO reference to that symbol -- its CPU test library links against a test double of the compute layer that
// does not have it: whisperImpl.cpp installs &wh_context_set_boost here when libWhisper.so is loaded, a test library installs its own. nullptr: a non-empty
// set in Whisper::setBatchBoostedPhrases answers E_NOTIMPL.
#pragma once
#include "whisper_hip.h"
#include <cstdint>

namespace Whisper
{
	using pfnBatchBoost = int ( * )( wh_context* c, const int32_t* tokens, const int32_t* lens, int count, int nMax, float boost );
	extern pfnBatchBoost g_batchBoost;
}
