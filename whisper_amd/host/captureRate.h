// A capture at another rate than 16 kHz, as capture.cpp reaches the device half of it: the three entry points a 16 kHz capture never calls
// (include/whisper_hip.h: wh_capture_create_rate, wh_capture_flush, wh_capture_skip). capture.cpp holds NO reference to those symbols -- the refusal driver of
// tests/test_capture_cpu.py links it against stubs of exactly the six wh_capture_* functions a 16 kHz capture uses --: whisperImpl.cpp installs the table when
// libWhisper.so is loaded, a test driver installs its own. nullptr: iContext::runCapture of a capture at another rate is E_NOTIMPL.
#pragma once
#include "hostCommon.h"

namespace Whisper
{
	struct CaptureRateTable
	{
		int ( *createRate )( wh_context* c, int channels, int keepStereo, int64_t capSamples, int inRate, wh_capture** out );
		int ( *flush )( wh_capture* cap, float* featHost, int64_t featCap, int64_t* nNewFrames );
		int ( *skip )( wh_capture* cap, int64_t frames, int64_t* nSkippedOutputs );
	};
	extern const CaptureRateTable* g_captureRateTable;

	constexpr uint32_t CAPTURE_MIN_RATE = 1000, CAPTURE_MAX_RATE = 384000;
}
