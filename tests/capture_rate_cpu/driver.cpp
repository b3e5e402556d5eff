// Stand-alone driver of the host session of a capture at another rate than 16 kHz for tests/test_capture_rate_cpu.py: whisper_amd/host/capture.cpp as it
// ships, with support.cpp (logging, status codes) over the CPU test double of the compute layer (tests/hostloop_cpu/fake_device.cpp), a context double whose
// runFull only counts (and, in one case, stays busy until the loop has discarded five reads), counting stubs of the six wh_capture_* entry points a 16 kHz
// capture uses, and a scripted table of the three a capture at another rate adds (captureRate.h). The scripted device:
//   - a 16 kHz object appends one sample per frame;
//   - an object made by the table's create appends ( frames - 7 ) / 3 samples for its first chunk and frames / 3 afterwards, 2 for the flush, and a skip of F
//     frames moves the clock by F / 3 + 1 (0 for no frames): numbers no chunk's frame count equals, so a clock that counted frames would show;
//   - frame 0 of a buffer is silent, every other frame is speech, so the loop fires at maxDuration and at the end of the stream;
//   - an append or a flush whose feature buffer is too small for the frames it completes fails.
// Built with the address and undefined-behaviour sanitizers. One line per case: name, HRESULT, calls of the six old entries "create,append,clear,take,size,
// destroy", calls of the table "create,flush,skip", pieces "start:count,...", the frame counts of the appends, those of the skips, skips of no frames, the log.
#include "hostCommon.h"
#include "captureRate.h"
#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>

using namespace Whisper;

struct wh_capture
{
	bool atRate = false, first = true;
	int64_t n = 0;
};

namespace
{
	int g_old[ 6 ] = {}, g_table[ 3 ] = {};
	std::vector<int64_t> g_appended, g_skipped;
	int g_zeroSkips = 0;
	std::vector<float> g_zeros( 600000, 0.0f );
	std::mutex g_mx;
	std::condition_variable g_cv;
	int g_skipsSeen = 0, g_piecesSeen = 0;
	bool g_busyFirstJob = false;

	// the features of the frames that `outputs` more samples complete
	int grow( wh_capture* p, int64_t outputs, float* feat, int64_t featCap, int64_t* nNew )
	{
		const int64_t lo = p->n / 256, hi = ( p->n + outputs ) / 256;
		if( featCap < hi - lo || ( hi > lo && !feat ) ) return WH_E_INVALIDARG;
		for( int64_t f = lo; f < hi; f++ )
		{
			float* const o = feat + 3 * ( f - lo );
			if( f == 0 ) { o[ 0 ] = 1.0f; o[ 1 ] = 0.0f; o[ 2 ] = 0.0f; }
			else { o[ 0 ] = 1000.0f; o[ 1 ] = 1000.0f; o[ 2 ] = 100.0f; }
		}
		p->n += outputs;
		*nNew = hi - lo;
		return 0;
	}

	int tableCreate( wh_context*, int, int, int64_t, int inRate, wh_capture** out )
	{
		g_table[ 0 ]++;
		*out = new wh_capture();
		( *out )->atRate = inRate != 16000;
		return 0;
	}
	int tableFlush( wh_capture* p, float* feat, int64_t featCap, int64_t* nNew )
	{
		g_table[ 1 ]++;
		return grow( p, 2, feat, featCap, nNew );
	}
	int tableSkip( wh_capture*, int64_t frames, int64_t* nSkipped )
	{
		g_table[ 2 ]++;
		g_skipped.push_back( frames );
		if( frames == 0 ) g_zeroSkips++;
		*nSkipped = frames > 0 ? frames / 3 + 1 : 0;
		std::unique_lock<std::mutex> lk( g_mx );
		g_skipsSeen++;
		g_cv.notify_all();
		// the fifth discarded read lets the busy job go and waits until its piece was reported, so that the stall ends here and not whenever the worker wakes
		if( g_busyFirstJob && g_skipsSeen == 5 ) g_cv.wait( lk, [] { return g_piecesSeen >= 1; } );
		return 0;
	}
	const CaptureRateTable g_scripted = { &tableCreate, &tableFlush, &tableSkip };
}

extern "C" {
int wh_capture_create( wh_context*, int, int, int64_t, wh_capture** out ) { g_old[ 0 ]++; *out = new wh_capture(); return 0; }
int wh_capture_append( wh_capture* p, const void*, int, int64_t frames, float* feat, int64_t featCap, int64_t* nNew )
{
	g_old[ 1 ]++;
	g_appended.push_back( frames );
	const int64_t outputs = !p->atRate ? frames : p->first ? ( frames - 7 ) / 3 : frames / 3;
	p->first = false;
	return grow( p, outputs, feat, featCap, nNew );
}
int wh_capture_clear( wh_capture* p ) { g_old[ 2 ]++; p->n = 0; return 0; }
int wh_capture_take( wh_capture* p, const float** mono, const float** stereo, int64_t* n )
{
	g_old[ 3 ]++;
	if( p->n > (int64_t)g_zeros.size() ) return WH_E_BOUNDS;
	*mono = g_zeros.data();
	if( stereo ) *stereo = nullptr;
	*n = p->n;
	p->n = 0;
	return 0;
}
int wh_capture_size( const wh_capture* p, int64_t* n ) { g_old[ 4 ]++; *n = p->n; return 0; }
int wh_capture_destroy( wh_capture* p ) { g_old[ 5 ]++; delete p; return 0; }
}

namespace
{
	class ContextDouble : public ComObject<iContext>
	{
	public:
		int runs = 0;
		bool firstJobWaitsForSkips = false;
		HRESULT runFull( const sFullParams&, const iAudioBuffer* ) override
		{
			runs++;
			if( firstJobWaitsForSkips && runs == 1 )
			{
				std::unique_lock<std::mutex> lk( g_mx );
				g_cv.wait( lk, [] { return g_skipsSeen >= 5; } );
			}
			return S_OK;
		}
		HRESULT runStreamed( const sFullParams&, const sProgressSink&, const iAudioReader* ) override { return E_NOTIMPL; }
		HRESULT runCapture( const sFullParams&, const sCaptureCallbacks&, const iAudioCapture* ) override { return E_NOTIMPL; }
		HRESULT getResults( eResultFlags, iTranscribeResult** ) const override { return E_NOTIMPL; }
		HRESULT detectSpeaker( const sTimeInterval&, eSpeakerChannel& ) const override { return E_NOTIMPL; }
		HRESULT getModel( iModel** ) override { return E_NOTIMPL; }
		HRESULT fullDefaultParams( eSamplingStrategy, sFullParams* ) override { return E_NOTIMPL; }
		HRESULT timingsPrint() override { return S_OK; }
		HRESULT timingsReset() override { return S_OK; }
	};

	std::string g_log, g_pieces;
	void sink( void*, eLogLevel, const char* message ) { g_log += message; g_log += " | "; }
	void piece( void*, int64_t start, int64_t count )
	{
		if( !g_pieces.empty() ) g_pieces += ",";
		g_pieces += std::to_string( start ) + ":" + std::to_string( count );
		{
			std::lock_guard<std::mutex> lk( g_mx );
			g_piecesSeen++;
		}
		g_cv.notify_all();
	}
	std::string csv( const int* v, int n )
	{
		std::string s;
		for( int i = 0; i < n; i++ ) s += ( i ? "," : "" ) + std::to_string( v[ i ] );
		return s;
	}
	std::string csv( const std::vector<int64_t>& v )
	{
		std::string s;
		for( size_t i = 0; i < v.size(); i++ ) s += ( i ? "," : "" ) + std::to_string( v[ i ] );
		return s;
	}

	// `chunks` writes of `frames` s16 mono frames into a capture at `rate` (0: Whisper::createPcmCapture), closed, then runCapture over the doubles
	void run( const char* name, uint32_t rate, uint32_t flags, int chunks, uint32_t frames, bool table, bool busyFirstJob, float minDuration = 2.0f, float maxDuration = 3.0f )
	{
		for( int& v : g_old ) v = 0;
		for( int& v : g_table ) v = 0;
		g_appended.clear();
		g_skipped.clear();
		g_zeroSkips = g_skipsSeen = g_piecesSeen = 0;
		g_busyFirstJob = busyFirstJob;
		g_pieces.clear();
		g_log.clear();
		g_captureRateTable = table ? &g_scripted : nullptr;

		sCaptureParams cp;
		cp.flags = flags;
		cp.minDuration = minDuration;
		cp.maxDuration = maxDuration;
		iPcmCapture* cap = nullptr;
		HRESULT hr = rate ? createPcmCaptureAtRate( cp, rate, &cap ) : createPcmCapture( cp, &cap );
		if( SUCCEEDED( hr ) )
		{
			const std::vector<int16_t> samples( frames, 0 );
			for( int i = 0; i < chunks && SUCCEEDED( hr ); i++ ) hr = cap->write( samples.data(), 1, 1, frames );
			cap->close();
		}
		ContextDouble* ctx = new ContextDouble();
		ctx->firstJobWaitsForSkips = busyFirstJob;
		if( SUCCEEDED( hr ) )
		{
			sFullParams p{};
			const sCaptureCallbacks cb{ nullptr, nullptr, nullptr };
			hr = runCaptureLoop( ctx, (wh_context*)(uintptr_t)16, p, cb, cap, &piece, nullptr );
		}
		if( cap ) cap->Release();
		ctx->Release();
		printf( "%s\t0x%08x\t%s\t%s\t%s\t%s\t%s\t%d\t%s\n", name, (unsigned)hr, csv( g_old, 6 ).c_str(), csv( g_table, 3 ).c_str(), g_pieces.c_str(), csv( g_appended ).c_str(),
			csv( g_skipped ).c_str(), g_zeroSkips, g_log.c_str() );
		fflush( stdout );
	}
}

int main()
{
	sLoggerSetup log{};
	log.sink = &sink;
	log.level = eLogLevel::Debug;
	setupLogger( log );
	const uint32_t noDrop = (uint32_t)eCaptureFlags::NoDrop;

	// 4 s of 16 kHz: the table is installed and never called
	run( "plain_16k", 0, noDrop, 40, 1600, true, false );
	run( "at_rate_16000", 16000, noDrop, 40, 1600, true, false );
	// 4 s of 48 kHz in writes of 100 ms
	run( "rate_48k", 48000, noDrop, 40, 4800, true, false );
	// 0.68 s of 48 kHz in writes of 10 ms without NoDrop, pieces of a quarter of a second: the first job stays busy until five reads were discarded. 26 reads fill the
	// first piece, 25 the second, which stalls; behind the stall fewer reads are left than fill a third, so the rest goes out at the end of the stream and no
	// later post depends on when a worker thread ends. (All of it is written before the loop runs; a queue without NoDrop holds maxDuration + 1 s, 125 such chunks.)
	run( "stall_48k", 48000, 0, 68, 480, true, true, 0.125f, 0.25f );
	// no table: not implemented, before any device call
	run( "no_table", 48000, noDrop, 4, 4800, false, false );

	const sCaptureParams cp;
	for( const uint32_t rate : { 999u, 1000u, 384000u, 384001u } )
	{
		iPcmCapture* cap = nullptr;
		const HRESULT hr = createPcmCaptureAtRate( cp, rate, &cap );
		printf( "create_%u\t0x%08x\n", rate, (unsigned)hr );
		if( cap ) cap->Release();
	}
	return 0;
}
