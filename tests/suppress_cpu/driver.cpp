// tests/suppress_cpu/driver.cpp -- a program of its own over whisper_amd/host/nonSpeechTokens.h, compiled alone (no other file of the project), also under
// -fsanitize=address,undefined (tests/test_suppress_cpu.py).
//   driver vocab.bin eot     vocab.bin = uint32 n, then n times { uint32 length, bytes }: the stored text of token 0 .. n - 1.
// Prints the number of symbols on the first line and the non-speech ids, blank-separated, on the second.
#include "nonSpeechTokens.h"
#include <cstdio>
#include <cstdlib>
#include <fstream>

int main( int argc, char** argv )
{
	if( argc < 3 ) { fprintf( stderr, "usage: %s vocab.bin eot\n", argv[ 0 ] ); return 2; }
	std::ifstream f( argv[ 1 ], std::ios::binary );
	uint32_t n = 0;
	f.read( (char*)&n, 4 );
	if( !f || n > ( 1u << 20 ) ) { fprintf( stderr, "bad vocabulary file\n" ); return 2; }
	std::vector<std::string> words( n );
	for( uint32_t i = 0; i < n; i++ )
	{
		uint32_t len = 0;
		f.read( (char*)&len, 4 );
		if( !f || len > 4096 ) { fprintf( stderr, "bad vocabulary file\n" ); return 2; }
		words[ i ].resize( len );
		if( len ) f.read( &words[ i ][ 0 ], len );
	}
	if( !f ) { fprintf( stderr, "bad vocabulary file\n" ); return 2; }
	const std::vector<int32_t> ids = Whisper::nonSpeechTokens( words, atoi( argv[ 2 ] ) );
	printf( "%d\n", (int)Whisper::nonSpeechSymbols().size() );
	for( size_t i = 0; i < ids.size(); i++ ) printf( i ? " %d" : "%d", (int)ids[ i ] );
	printf( "\n" );
	return 0;
}
