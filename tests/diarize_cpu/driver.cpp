// Stand-alone driver of whisper_amd/host/diarize.h for tests/test_diarize_cpu.py (built with -fsanitize=address,undefined and run as a program).
//   driver <file>   one line per case of the file: "<HRESULT as 8 hex digits> <eSpeakerChannel as a decimal number>"
// A case in the file (little endian): int64 frames (-1 = no stereo data: a null pointer), int64 mediaTimeOffset, uint64 begin ticks, uint64 end ticks,
// then frames * 2 float32. The PCM of every case sits in a heap block of exactly its size, so a slice that is read past the end of the buffer, or before its
// start, is something the sanitizer reports. "chunk <ticks> <offset>" instead of a file prints chunkOffset.
#include "diarize.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main( int argc, char** argv )
{
	if( argc == 4 && !strcmp( argv[ 1 ], "chunk" ) )
	{
		printf( "%lld\n", (long long)Whisper::diarize::chunkOffset( atoll( argv[ 2 ] ), atoll( argv[ 3 ] ) ) );
		return 0;
	}
	if( argc != 2 ) { fprintf( stderr, "usage: driver <file> | driver chunk <ticks> <offset>\n" ); return 1; }
	FILE* f = fopen( argv[ 1 ], "rb" );
	if( !f ) { fprintf( stderr, "cannot open %s\n", argv[ 1 ] ); return 1; }
	while( true )
	{
		int64_t head[ 4 ];
		const size_t got = fread( head, 1, sizeof( head ), f );
		if( got == 0 ) break;
		if( got != sizeof( head ) || head[ 0 ] < -1 ) { fprintf( stderr, "bad case header\n" ); return 1; }
		float* pcm = nullptr;
		const size_t frames = head[ 0 ] < 0 ? 0 : (size_t)head[ 0 ];
		if( head[ 0 ] >= 0 )
		{
			// malloc( 0 ) may be null: one byte, so that "zero frames of stereo data" stays apart from "no stereo data"
			pcm = (float*)malloc( frames ? frames * 2 * sizeof( float ) : 1 );
			if( !pcm || fread( pcm, 2 * sizeof( float ), frames, f ) != frames ) { fprintf( stderr, "short read\n" ); return 1; }
		}
		Whisper::sTimeInterval time;
		time.begin.ticks = (uint64_t)head[ 2 ];
		time.end.ticks = (uint64_t)head[ 3 ];
		Whisper::eSpeakerChannel ch = (Whisper::eSpeakerChannel)0x7E;	   // neither a verdict nor NoStereoData: what a failed call leaves
		const HRESULT hr = Whisper::diarize::detectSpeaker( pcm, frames, head[ 1 ], time, ch );
		printf( "%08X %u\n", (unsigned)hr, (unsigned)(uint8_t)ch );
		free( pcm );
	}
	fclose( f );
	return 0;
}
