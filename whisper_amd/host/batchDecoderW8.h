// INT8 decoder weights in the lock-step batch runner ("INT8 decoder weights"; sBatchSetup::flags bit value 16): how the scheduler turns the
// setting on for a group's context, the signature of wh_context_set_decoder_w8. batchScheduler.cpp holds NO reference to that symbol -- its CPU test library links
// against a test double of the compute layer that does not have it: whisperImpl.cpp installs &wh_context_set_decoder_w8 here when libWhisper.so is loaded.
// nullptr: createBatchRunner with the bit set answers E_NOTIMPL.
#pragma once
#include "whisper_hip.h"

namespace Whisper
{
	using pfnBatchSetDecoderW8 = int ( * )( wh_context* c, int on );
	extern pfnBatchSetDecoderW8 g_batchSetDecoderW8;
}
