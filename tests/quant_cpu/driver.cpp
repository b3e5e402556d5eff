// Stand-alone driver of whisper_amd/host/ggmlTensor.h for tests/test_quant_cpu.py (built with -fsanitize=address,undefined and run as a program).
//   driver payload <type> <f16 of the header> <ne0> [<ne1> [<ne2>]]   ->  "ok <count> <bytes>"        exit 0
//                                                                      or  "rejected: <text>"         exit 2
//   driver header <f16>                                                ->  "<qntvr> <ftype> <words>"  exit 0
//   driver block <type>                                                ->  "<bytes of a block, 0 = not quantized> <name>"
#include "ggmlTensor.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main( int argc, char** argv )
{
	using namespace Whisper;
	if( argc == 3 && !strcmp( argv[ 1 ], "header" ) )
	{
		const int32_t f16 = (int32_t)strtol( argv[ 2 ], nullptr, 10 );
		const ggml::FileType t = ggml::splitFileType( f16 );
		printf( "%d %d %s\n", t.qntvr, t.ftype, ggml::describeFileType( f16 ).c_str() );
		return 0;
	}
	if( argc == 3 && !strcmp( argv[ 1 ], "block" ) )
	{
		const int type = (int)strtol( argv[ 2 ], nullptr, 10 );
		printf( "%d %s\n", ggml::blockBytes( type ), ggml::typeName( type ) );
		return 0;
	}
	if( argc >= 5 && argc <= 7 && !strcmp( argv[ 1 ], "payload" ) )
	{
		const int type = (int)strtol( argv[ 2 ], nullptr, 10 );
		const int32_t f16 = (int32_t)strtol( argv[ 3 ], nullptr, 10 );
		// exactly nDims ints on the heap: a reader of ne[ nDims ] is reported
		const int nDims = argc - 4;
		int32_t* const ne = (int32_t*)malloc( sizeof( int32_t ) * (size_t)nDims );
		for( int i = 0; i < nDims; i++ ) ne[ i ] = (int32_t)strtoll( argv[ 4 + i ], nullptr, 10 );
		int64_t count = -1, bytes = -1;
		std::string error;
		int rc = 0;
		if( ggml::payloadBytes( type, nDims, ne, f16, count, bytes, error ) )
			printf( "ok %lld %lld\n", (long long)count, (long long)bytes );
		else
		{
			printf( "rejected: %s\n", error.c_str() );
			rc = 2;
		}
		free( ne );
		return rc;
	}
	fprintf( stderr, "usage: driver payload <type> <f16> <ne0> [<ne1> [<ne2>]] | header <f16> | block <type>\n" );
	return 1;
}
