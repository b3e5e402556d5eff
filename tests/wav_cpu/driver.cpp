// Stand-alone driver of whisper_amd/host/wavFormat.h for tests/test_resample_cpu.py (built with -fsanitize=address,undefined and run as a program).
//   driver <file>   ->  "ok <format> <channels> <rate> <firstByte> <frames> <sum of all samples as floats, %.9g>"   exit 0
//                   or  "rejected: <text>"                                                                          exit 2
// The file sits in a heap block of exactly its size, and every sample the header promises is converted: a parser that trusts a length in the file reads
// outside the block, which the sanitizer reports.
#include "wavFormat.h"
#include <cstdlib>
#include <cstring>

int main( int argc, char** argv )
{
	if( argc != 2 ) { fprintf( stderr, "usage: driver <file>\n" ); return 1; }
	FILE* f = fopen( argv[ 1 ], "rb" );
	if( !f ) { fprintf( stderr, "cannot open %s\n", argv[ 1 ] ); return 1; }
	fseek( f, 0, SEEK_END );
	const long size = ftell( f );
	fseek( f, 0, SEEK_SET );
	unsigned char* const bytes = (unsigned char*)malloc( (size_t)size );
	if( size > 0 && fread( bytes, 1, (size_t)size, f ) != (size_t)size ) { fprintf( stderr, "short read\n" ); return 1; }
	fclose( f );

	Whisper::wav::Info info;
	std::string error;
	int rc = 0;
	if( Whisper::wav::parse( bytes, (size_t)size, info, error ) )
	{
		const size_t step = (size_t)Whisper::wav::bytesPerSample( info.format );
		double sum = 0.0;
		for( size_t i = 0; i < info.frames * (size_t)info.channels; i++ ) sum += (double)Whisper::wav::sample( bytes + info.firstByte + i * step, info.format );
		printf( "ok %d %d %d %zu %zu %.9g\n", info.format, info.channels, info.rate, info.firstByte, info.frames, sum );
	}
	else
	{
		printf( "rejected: %s\n", error.c_str() );
		rc = 2;
	}
	free( bytes );
	return rc;
}
