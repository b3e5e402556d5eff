// Stand-alone driver of whisper_amd/host/speechSpans.h for tests/test_speech_spans_cpu.py (built with -fsanitize=address,undefined and run as a program).
//   driver spans <file> <N> <minSilence> <minSpeech> <pad>      file: nFrames flag bytes
//        ->  "ok <count>" and one "<a> <b>" line per span, or "failed 0x<hresult>"
//   driver map <file> <N> <minSilence> <minSpeech> <pad> <queries>   queries: a file of int64 tick values
//        ->  the spans as above, then "packed <length>", then per query "<startTicks> <endTicks> <start of t div 625> <end of t div 625>"
// The flags sit in a heap block of exactly their size: a loop that runs past the frames it was given reads outside the block, which the sanitizer reports.
#include "speechSpans.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static bool readAll( const char* path, unsigned char*& bytes, size_t& size )
{
	FILE* f = fopen( path, "rb" );
	if( !f ) { fprintf( stderr, "cannot open %s\n", path ); return false; }
	fseek( f, 0, SEEK_END );
	size = (size_t)ftell( f );
	fseek( f, 0, SEEK_SET );
	bytes = (unsigned char*)malloc( size ? size : 1 );
	const bool ok = size == 0 || fread( bytes, 1, size, f ) == size;
	fclose( f );
	if( !ok ) fprintf( stderr, "short read\n" );
	return ok;
}

int main( int argc, char** argv )
{
	using namespace Whisper::speechRules;
	const bool map = argc == 8 && 0 == strcmp( argv[ 1 ], "map" );
	if( !map && !( argc == 7 && 0 == strcmp( argv[ 1 ], "spans" ) ) )
	{
		fprintf( stderr, "usage: driver spans <file> <N> <minSilence> <minSpeech> <pad> | map <file> <N> <minSilence> <minSpeech> <pad> <queries>\n" );
		return 1;
	}
	unsigned char* bytes = nullptr;
	size_t size = 0;
	if( !readAll( argv[ 2 ], bytes, size ) ) return 1;
	std::vector<Span> spans;
	const HRESULT hr = find( size ? bytes : nullptr, (int64_t)size, atoll( argv[ 3 ] ), atoll( argv[ 4 ] ), atoll( argv[ 5 ] ), atoll( argv[ 6 ] ), spans );
	free( bytes );
	if( FAILED( hr ) ) { printf( "failed 0x%08x\n", (unsigned)hr ); return 0; }
	printf( "ok %zu\n", spans.size() );
	for( const Span& s : spans ) printf( "%lld %lld\n", (long long)s.a, (long long)s.b );
	if( !map ) return 0;
	unsigned char* q = nullptr;
	size_t qSize = 0;
	if( !readAll( argv[ 7 ], q, qSize ) ) return 1;
	const TimeMap tm( spans );
	printf( "packed %lld\n", (long long)tm.packedLength() );
	if( tm.packedLength() != packedLength( spans ) ) return 3;
	for( size_t i = 0; i + 8 <= qSize; i += 8 )
	{
		int64_t t = 0;
		memcpy( &t, q + i, 8 );
		printf( "%lld %lld %lld %lld\n", (long long)tm.startTicks( t ), (long long)tm.endTicks( t ), (long long)tm.start( t / TICKS_PER_SAMPLE ),
			(long long)tm.end( t / TICKS_PER_SAMPLE ) );
	}
	free( q );
	return 0;
}
