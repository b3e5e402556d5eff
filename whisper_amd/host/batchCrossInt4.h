// INT4 cross-attention caches in the lock-step batch runner ("INT4 cross-attention caches"; sBatchSetup::flags bit value 8): how the scheduler
// creates a group's context, the signature of wh_context_create_kv4. As with batchCrossFp8.h, batchScheduler.cpp holds NO reference to that symbol: whisperImpl.cpp
// installs &wh_context_create_kv4 here when libWhisper.so is loaded. nullptr: createBatchRunner with the bit set answers E_NOTIMPL.
#pragma once
#include "whisper_hip.h"

namespace Whisper
{
	using pfnBatchCreateKv4 = int ( * )( wh_model* m, int maxBatch, void* stream, wh_context** out );
	extern pfnBatchCreateKv4 g_batchCreateKv4;
}
