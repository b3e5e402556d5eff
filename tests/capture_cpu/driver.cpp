// Stand-alone driver of whisper_amd/host/captureLoop.h (and the resumable detector of vad.h) for tests/test_capture_cpu.py: the header alone, no device, no
// library; built with the address and undefined-behaviour sanitizers. Everything the loop leaves open is scripted here:
//   loop MIN MAX DROP PAUSE FLAGS CANCEL_AT CHUNKS INTERVALS JOBS [worker]
//     durations in seconds; CANCEL_AT: the pass whose cancel check stops the loop, -1 never; CHUNKS: "NxK,N,..." sizes of the reads (N repeated K times);
//     INTERVALS: "a-b,..." stream samples that are speech, "-" for none: frame f of a buffer that begins at `start` is speech when start + 256 f lies in one;
//     JOBS: "d,..." job k, posted in pass P, is found ended by a poll in pass >= P + d ("-": every job 0).
//     worker: the job's end is also announced the way a worker thread does it, Loop::workerEnded(), at the start of the pass in which a poll would find it.
//     prints "hr 0x..", "status w w ..", "pieces a-b ..", "discarded a-b .."
//   samples SECONDS...      prints samplesFromSeconds of each
//   validate MIN MAX        prints validate's HRESULT
//   vad FILE SPLITS         FILE: float32 [n][3] features; SPLITS: "NxK,.." frames per feed; prints "lastSpeech of the splits" "decide's" "flags equal"
#include "captureLoop.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace Whisper;

static std::vector<int64_t> parseList( const char* s )
{
	std::vector<int64_t> out;
	if( !s || !strcmp( s, "-" ) ) return out;
	while( *s )
	{
		char* e = nullptr;
		const long long v = strtoll( s, &e, 10 );
		long long k = 1;
		if( *e == 'x' ) k = strtoll( e + 1, &e, 10 );
		for( long long i = 0; i < k; i++ ) out.push_back( v );
		s = *e == ',' ? e + 1 : e;
	}
	return out;
}
static std::vector<std::pair<int64_t, int64_t>> parseIntervals( const char* s )
{
	std::vector<std::pair<int64_t, int64_t>> out;
	if( !s || !strcmp( s, "-" ) ) return out;
	while( *s )
	{
		char* e = nullptr;
		const long long a = strtoll( s, &e, 10 );
		const long long b = strtoll( e + 1, &e, 10 );
		out.push_back( { a, b } );
		s = *e == ',' ? e + 1 : e;
	}
	return out;
}

static int runLoop( char** a, bool worker )
{
	sCaptureParams cp;
	cp.minDuration = strtof( a[ 0 ], nullptr );
	cp.maxDuration = strtof( a[ 1 ], nullptr );
	cp.dropStartSilence = strtof( a[ 2 ], nullptr );
	cp.pauseDuration = strtof( a[ 3 ], nullptr );
	cp.flags = (uint32_t)strtoul( a[ 4 ], nullptr, 0 );
	const long long cancelAt = strtoll( a[ 5 ], nullptr, 10 );
	const std::vector<int64_t> chunks = parseList( a[ 6 ] );
	const auto intervals = parseIntervals( a[ 7 ] );
	const std::vector<int64_t> jobs = parseList( a[ 8 ] );

	long long pass = -1;
	size_t nextChunk = 0;
	int64_t nextSample = 0, bufStart = 0;
	long long jobPosted = 0;
	size_t jobCount = 0;
	std::vector<int> status;
	std::vector<std::pair<int64_t, int64_t>> pieces, discarded;
	const float noFeatures[ 3 ] = { 0, 0, 0 };

	captureLoop::Hooks h;
	captureLoop::Loop* running = nullptr;
	bool announced = true;
	h.shouldCancel = [ & ]() -> HRESULT {
		pass++;
		if( worker && !announced && running )
		{
			const long long d = jobCount - 1 < jobs.size() ? jobs[ jobCount - 1 ] : 0;
			if( pass >= jobPosted + d ) { announced = true; running->workerEnded(); }
		}
		return pass == cancelAt ? S_FALSE : S_OK;
	};
	h.status = [ & ]( uint8_t w ) -> HRESULT { status.push_back( w ); return S_OK; };
	h.read = [ & ]( bool discard, uint32_t& frames, const float*& feat, int64_t& newFrames ) -> HRESULT {
		if( nextChunk >= chunks.size() ) return S_FALSE;
		frames = (uint32_t)chunks[ nextChunk++ ];
		if( discard ) discarded.push_back( { nextSample, nextSample + frames } );
		nextSample += frames;
		feat = noFeatures;
		newFrames = 0;
		return S_OK;
	};
	h.vadStep = [ & ]( const float*, int64_t, int64_t bufferSamples ) -> int64_t {
		int64_t last = 0;
		for( int64_t f = 0; f < bufferSamples / vad::FRAME_SAMPLES; f++ )
		{
			const int64_t s = bufStart + vad::FRAME_SAMPLES * f;
			for( const auto& iv : intervals )
				if( s >= iv.first && s < iv.second ) last = ( f + 1 ) * vad::FRAME_SAMPLES;
		}
		return last;
	};
	h.vadClear = []() {};
	h.dropBuffer = [ & ]() { bufStart = nextSample; };
	h.post = [ & ]( int64_t start, int64_t count ) -> HRESULT {
		if( start != bufStart ) { printf( "post: start %lld, the driver's buffer begins at %lld\n", (long long)start, (long long)bufStart ); return E_UNEXPECTED; }
		pieces.push_back( { start, start + count } );
		bufStart = nextSample;
		jobPosted = pass;
		jobCount++;
		announced = false;
		return S_OK;
	};
	h.jobPoll = [ & ]() -> HRESULT {
		const long long d = jobCount - 1 < jobs.size() ? jobs[ jobCount - 1 ] : 0;
		return pass >= jobPosted + d ? S_OK : S_FALSE;
	};
	h.jobWait = []() -> HRESULT { return S_OK; };

	const char* which = nullptr;
	HRESULT hr = captureLoop::validate( cp, &which );
	if( SUCCEEDED( hr ) )
	{
		captureLoop::Loop loop( captureLoop::Params( cp ), h );
		running = &loop;
		hr = loop.run();
	}
	printf( "hr 0x%08x\nstatus", (unsigned)hr );
	for( int w : status ) printf( " %d", w );
	printf( "\npieces" );
	for( const auto& p : pieces ) printf( " %lld-%lld", (long long)p.first, (long long)p.second );
	printf( "\ndiscarded" );
	for( const auto& p : discarded ) printf( " %lld-%lld", (long long)p.first, (long long)p.second );
	printf( "\n" );
	return 0;
}

static int runVad( const char* path, const char* splits )
{
	FILE* f = fopen( path, "rb" );
	if( !f ) return 2;
	std::vector<float> feat;
	float row[ 3 ];
	while( fread( row, sizeof( float ), 3, f ) == 3 ) feat.insert( feat.end(), row, row + 3 );
	fclose( f );
	const int64_t n = (int64_t)feat.size() / 3;
	std::vector<uint8_t> whole( (size_t)n + 1 ), parts( (size_t)n + 1 );
	const int64_t want = vad::decide( feat.data(), n, whole.data() );
	captureLoop::DetectorStep d;
	int64_t got = 0, done = 0;
	for( int64_t k : parseList( splits ) )
	{
		if( done + k > n ) k = n - done;
		// the buffer behind the feed holds the frames fed so far
		got = d.step( feat.data() + 3 * done, k, ( done + k ) * vad::FRAME_SAMPLES, parts.data() + done );
		done += k;
	}
	if( done < n ) got = d.step( feat.data() + 3 * done, n - done, n * vad::FRAME_SAMPLES, parts.data() + done );
	printf( "%lld %lld %d\n", (long long)got, (long long)want, 0 == memcmp( whole.data(), parts.data(), (size_t)n ) ? 1 : 0 );
	return 0;
}

int main( int argc, char** argv )
{
	if( argc >= 11 && !strcmp( argv[ 1 ], "loop" ) ) return runLoop( argv + 2, argc >= 12 && !strcmp( argv[ 11 ], "worker" ) );
	if( argc >= 3 && !strcmp( argv[ 1 ], "samples" ) )
	{
		for( int i = 2; i < argc; i++ ) printf( "%u\n", captureLoop::samplesFromSeconds( strtof( argv[ i ], nullptr ) ) );
		return 0;
	}
	if( argc == 4 && !strcmp( argv[ 1 ], "validate" ) )
	{
		sCaptureParams cp;
		cp.minDuration = strtof( argv[ 2 ], nullptr );
		cp.maxDuration = strtof( argv[ 3 ], nullptr );
		printf( "0x%08x\n", (unsigned)captureLoop::validate( cp ) );
		return 0;
	}
	if( argc == 4 && !strcmp( argv[ 1 ], "vad" ) ) return runVad( argv[ 2 ], argv[ 3 ] );
	fprintf( stderr, "usage: see the head of tests/capture_cpu/driver.cpp\n" );
	return 2;
}
