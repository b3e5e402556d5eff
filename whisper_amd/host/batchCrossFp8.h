// FP8 cross-attention caches in the lock-step batch runner ("FP8 cross-attention caches"; sBatchSetup::flags bit 2): how the scheduler creates
// a group's context, the signature of wh_context_create_kv8. batchScheduler.cpp holds NO reference to that symbol -- its CPU test library links against a test
// double of the compute layer that does not have it: whisperImpl.cpp installs &wh_context_create_kv8 here when libWhisper.so is loaded. nullptr: createBatchRunner
// with the bit set answers E_NOTIMPL.
#pragma once
#include "whisper_hip.h"

namespace Whisper
{
	using pfnBatchCreateKv8 = int ( * )( wh_model* m, int maxBatch, void* stream, wh_context** out );
	extern pfnBatchCreateKv8 g_batchCreateKv8;
}
