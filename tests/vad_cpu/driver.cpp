// Stand-alone driver of whisper_amd/host/vad.h and chunkPlanner.h for tests/test_vad_cpu.py (built with -fsanitize=address,undefined and run as a program).
//   driver decide <file>                                   file: float32 [nFrames][3] = energy, F, SFM
//        ->  "<nFrames> <lastSpeech>" and a line of nFrames characters 0 / 1
//   driver plan <file> <N> <maxLen> <minLen> <pauseFrames>  file: nFrames flag bytes, then nFrames float32 energies (nFrames = size / 5)
//        ->  "ok <count>" and one "<firstSample> <countSamples>" line per chunk, or "failed 0x<hresult>"
// Every array sits in a heap block of exactly its size: a loop that runs past the frames it was given reads outside the block, which the sanitizer reports.
#include "chunkPlanner.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

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
	if( argc < 3 ) { fprintf( stderr, "usage: driver decide <file> | plan <file> <N> <maxLen> <minLen> <pauseFrames>\n" ); return 1; }
	unsigned char* bytes = nullptr;
	size_t size = 0;
	if( !readAll( argv[ 2 ], bytes, size ) ) return 1;
	int rc = 0;
	if( 0 == strcmp( argv[ 1 ], "decide" ) && size % 12 == 0 )
	{
		const int64_t nFrames = (int64_t)( size / 12 );
		float* const feat = (float*)malloc( size ? size : 1 );
		memcpy( feat, bytes, size );
		uint8_t* const speech = (uint8_t*)malloc( nFrames ? (size_t)nFrames : 1 );
		const int64_t lastSpeech = Whisper::vad::decide( feat, nFrames, speech );
		std::string line;
		for( int64_t i = 0; i < nFrames; i++ ) line += speech[ i ] ? '1' : '0';
		printf( "%lld %lld\n%s\n", (long long)nFrames, (long long)lastSpeech, line.c_str() );
		// without the flags: the same answer
		if( Whisper::vad::decide( feat, nFrames, nullptr ) != lastSpeech ) rc = 3;
		free( speech );
		free( feat );
	}
	else if( 0 == strcmp( argv[ 1 ], "plan" ) && argc == 7 && size % 5 == 0 )
	{
		const int64_t nFrames = (int64_t)( size / 5 );
		uint8_t* const speech = (uint8_t*)malloc( nFrames ? (size_t)nFrames : 1 );
		float* const energy = (float*)malloc( nFrames ? (size_t)nFrames * 4 : 1 );
		memcpy( speech, bytes, (size_t)nFrames );
		memcpy( energy, bytes + nFrames, (size_t)nFrames * 4 );
		std::vector<Whisper::chunkPlanner::Chunk> chunks;
		const HRESULT hr = Whisper::chunkPlanner::plan( speech, energy, nFrames, atoll( argv[ 3 ] ), atoll( argv[ 4 ] ), atoll( argv[ 5 ] ), atoll( argv[ 6 ] ), chunks );
		if( FAILED( hr ) ) printf( "failed 0x%08x\n", (unsigned)hr );
		else
		{
			printf( "ok %zu\n", chunks.size() );
			for( const auto& c : chunks ) printf( "%lld %lld\n", (long long)c.firstSample, (long long)c.countSamples );
		}
		free( energy );
		free( speech );
	}
	else
	{
		fprintf( stderr, "bad arguments\n" );
		rc = 1;
	}
	free( bytes );
	return rc;
}
