// No-repeat n-grams in the lock-step batch runner ("No-repeat n-grams"): the device half as the scheduler reaches it, the signature of
// wh_context_set_no_repeat. batchScheduler.cpp holds NO reference to that symbol -- its CPU test library links against a test double of the compute layer that
// does not have it: whisperImpl.cpp installs &wh_context_set_no_repeat here when libWhisper.so is loaded, a test library installs its own. nullptr: turning the
// option on in Whisper::setBatchNoRepeatNgram answers E_NOTIMPL.
#pragma once
#include "whisper_hip.h"

namespace Whisper
{
	using pfnBatchNoRepeat = int ( * )( wh_context* c, int n );
	extern pfnBatchNoRepeat g_batchNoRepeat;
}
