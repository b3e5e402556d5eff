// Suppressed tokens in the lock-step batch runner ("Suppressed tokens"): the device half as the scheduler reaches it, the signature of
// wh_context_set_suppress. batchScheduler.cpp holds NO reference to that symbol -- its CPU test library links against a test double of the compute layer that
// does not have it: whisperImpl.cpp installs &wh_context_set_suppress here when libWhisper.so is loaded, a test library installs its own. nullptr: a non-empty
// set in Whisper::setBatchSuppressedTokens answers E_NOTIMPL.
#pragma once
#include "whisper_hip.h"
#include <cstdint>

namespace Whisper
{
	using pfnBatchSuppress = int ( * )( wh_context* c, const int32_t* ids, int count );
	extern pfnBatchSuppress g_batchSuppress;
}
