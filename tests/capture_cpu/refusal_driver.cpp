// Stand-alone driver of iContext::runCapture's refusals for tests/test_capture_cpu.py: whisper_amd/host/capture.cpp as it ships, with support.cpp (logging,
// status codes) over the CPU test double of the compute layer the host-loop tests use (tests/hostloop_cpu/fake_device.cpp), a context double that counts
// its runFull calls, and the wh_capture_* entry points -- which that double does not have -- as counting stubs that fail: a refusal must come before any of
// them is called. Built with the address and undefined-behaviour sanitizers. Prints one line per case: name, HRESULT, what was logged.
#include "hostCommon.h"
#include <cmath>
#include <cstdio>
#include <string>

using namespace Whisper;

static int g_deviceCalls = 0;
extern "C" {
int wh_capture_create( wh_context*, int, int, int64_t, wh_capture** out ) { g_deviceCalls++; if( out ) *out = nullptr; return WH_E_NO_DEVICE; }
int wh_capture_append( wh_capture*, const void*, int, int64_t, float*, int64_t, int64_t* ) { g_deviceCalls++; return WH_E_NO_DEVICE; }
int wh_capture_clear( wh_capture* ) { g_deviceCalls++; return WH_E_NO_DEVICE; }
int wh_capture_take( wh_capture*, const float**, const float**, int64_t* ) { g_deviceCalls++; return WH_E_NO_DEVICE; }
int wh_capture_size( const wh_capture*, int64_t* ) { g_deviceCalls++; return WH_E_NO_DEVICE; }
int wh_capture_destroy( wh_capture* ) { g_deviceCalls++; return 0; }
}

namespace
{
	// an iContext that only counts: runCaptureLoop calls nothing of it but runFull, from its worker
	class ContextDouble : public ComObject<iContext>
	{
	public:
		int runs = 0;
		HRESULT runFull( const sFullParams&, const iAudioBuffer* ) override { runs++; return S_OK; }
		HRESULT runStreamed( const sFullParams&, const sProgressSink&, const iAudioReader* ) override { return E_NOTIMPL; }
		HRESULT runCapture( const sFullParams& p, const sCaptureCallbacks& cb, const iAudioCapture* reader ) override
		{
			// what ContextImpl::runCapture does, with a device context that is never looked into
			return runCaptureLoop( this, (wh_context*)(uintptr_t)16, p, cb, reader, nullptr, nullptr );
		}
		HRESULT getResults( eResultFlags, iTranscribeResult** ) const override { return E_NOTIMPL; }
		HRESULT detectSpeaker( const sTimeInterval&, eSpeakerChannel& ) const override { return E_NOTIMPL; }
		HRESULT getModel( iModel** ) override { return E_NOTIMPL; }
		HRESULT fullDefaultParams( eSamplingStrategy, sFullParams* ) override { return E_NOTIMPL; }
		HRESULT timingsPrint() override { return S_OK; }
		HRESULT timingsReset() override { return S_OK; }
	};

	// a capture of another library: the reference's interface and nothing else
	class ForeignCapture : public ComObject<iAudioCapture>
	{
		sCaptureParams params;
	public:
		HRESULT getReader( IMFSourceReader** pp ) const override { if( pp ) *pp = nullptr; return E_NOTIMPL; }
		const sCaptureParams& getParams() const override { return params; }
	};

	std::string g_log;
	void sink( void*, eLogLevel, const char* message ) { g_log += message; g_log += " | "; }

	void report( const char* name, HRESULT hr, const ContextDouble& ctx )
	{
		printf( "%s\t0x%08x\t%d\t%d\t%s\n", name, (unsigned)hr, g_deviceCalls, ctx.runs, g_log.c_str() );
		g_log.clear();
	}
}

int main()
{
	sLoggerSetup log{};
	log.sink = &sink;
	log.level = eLogLevel::Debug;
	setupLogger( log );

	ContextDouble* ctx = new ContextDouble();
	sFullParams p{};
	const sCaptureCallbacks cb{ nullptr, nullptr, nullptr };

	report( "null", ctx->runCapture( p, cb, nullptr ), *ctx );

	ForeignCapture* foreign = new ForeignCapture();
	report( "foreign", ctx->runCapture( p, cb, foreign ), *ctx );
	foreign->Release();

	const struct { const char* name; float minD, maxD; } bad[] = { { "min_low", 0.1f, 3.0f }, { "min_high", 30.5f, 3.0f }, { "max_low", 2.0f, 0.1f }, { "max_high", 2.0f, 31.0f },
		{ "min_nan", NAN, 3.0f }, { "max_nan", 2.0f, NAN } };
	for( const auto& b : bad )
	{
		sCaptureParams cp;
		cp.minDuration = b.minD;
		cp.maxDuration = b.maxD;
		iPcmCapture* cap = nullptr;
		if( FAILED( createPcmCapture( cp, &cap ) ) ) return 3;
		report( b.name, ctx->runCapture( p, cb, cap ), *ctx );
		cap->Release();
	}

	// the edges of the ranges are legal, and a stream that ends before its first chunk is no error: still no device call
	{
		sCaptureParams cp;
		cp.minDuration = 0.125f;
		cp.maxDuration = 30.0f;
		cp.dropStartSilence = NAN;		// counts as 0
		cp.pauseDuration = -1.0f;
		iPcmCapture* cap = nullptr;
		if( FAILED( createPcmCapture( cp, &cap ) ) ) return 3;
		cap->close();
		report( "empty", ctx->runCapture( p, cb, cap ), *ctx );
		// a second loop on a capture is legal once the first has returned
		report( "empty_again", ctx->runCapture( p, cb, cap ), *ctx );
		cap->Release();
	}

	// a chunk reaches the device layer, whose failure is the call's: the stubs answer WH_E_NO_DEVICE
	{
		iPcmCapture* cap = nullptr;
		if( FAILED( createPcmCapture( sCaptureParams{}, &cap ) ) ) return 3;
		const int16_t samples[ 512 ] = {};
		if( FAILED( cap->write( samples, 1, 1, 512 ) ) ) return 4;
		cap->close();
		report( "device_failure", ctx->runCapture( p, cb, cap ), *ctx );
		cap->Release();
	}
	ctx->Release();
	return 0;
}
