// Timestamp rules in the lock-step batch runner ("Timestamp rules"): the device half as the scheduler reaches it, the signature of
// wh_context_set_timestamp_rules. batchScheduler.cpp holds NO reference to that symbol -- its CPU test library links against a test double of the compute layer
// that does not have it: whisperImpl.cpp installs &wh_context_set_timestamp_rules here when libWhisper.so is loaded, a test library installs its own. nullptr:
// turning the rules on in Whisper::setBatchTimestampRules answers E_NOTIMPL.
#pragma once
#include "whisper_hip.h"

namespace Whisper
{
	using pfnBatchTimestampRules = int ( * )( wh_context* c, int on );
	extern pfnBatchTimestampRules g_batchTimestampRules;
}
