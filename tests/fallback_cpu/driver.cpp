// Stand-alone driver of whisper_amd/host/decodeFallback.h for tests/test_fallback_cpu.py (built plain and with -fsanitize=address,undefined, run as a program).
//   driver schedule <inc>            ->  one line: the temperatures, %.9g
//   driver verdict <file>            file: "inc lpt et nth seed" / "scanFailed noSpeech resultLen n" / n lines "id p"
//        ->  "<avgLogprob %.17g> <entropy %.17g> <failed 0|1> <silent 0|1>"
//   driver plan <file>               file: "inc lpt et nth seed seek" / one line per attempt "scanFailed resultLen avgLogprob entropy noSpeech"
//        ->  per attempt judged "<index> <temperature %.9g> <nonce> <attempts> <verdict 0..3>", until a verdict other than Retry or the lines run out
// The tokens sit in a heap block of exactly their size: a score that reads outside [0, resultLen) of a shorter list is the sanitizer's to report.
#include "decodeFallback.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace Whisper;

struct Token
{
	int id;
	float p;
};

static bool readParams( FILE* f, sDecodingFallback& p, long long* seek )
{
	double inc, lpt, et, nth;
	unsigned long long seed;
	if( fscanf( f, "%lf %lf %lf %lf %llu", &inc, &lpt, &et, &nth, &seed ) != 5 ) return false;
	p.temperatureInc = (float)inc; p.logprobThold = (float)lpt; p.entropyThold = (float)et; p.noSpeechThold = (float)nth; p.seed = seed;
	if( seek && fscanf( f, "%lld", seek ) != 1 ) return false;
	return true;
}

int main( int argc, char** argv )
{
	if( argc < 3 ) { fprintf( stderr, "usage: driver schedule <inc> | verdict <file> | plan <file>\n" ); return 1; }
	if( 0 == strcmp( argv[ 1 ], "schedule" ) )
	{
		const std::vector<float> t = fallback::schedule( strtof( argv[ 2 ], nullptr ) );
		for( size_t i = 0; i < t.size(); i++ ) printf( "%s%.9g", i ? " " : "", (double)t[ i ] );
		printf( "\n" );
		return 0;
	}
	FILE* const f = fopen( argv[ 2 ], "r" );
	if( !f ) { fprintf( stderr, "cannot open %s\n", argv[ 2 ] ); return 1; }
	int rc = 0;
	sDecodingFallback params;
	if( 0 == strcmp( argv[ 1 ], "verdict" ) )
	{
		int scanFailed = 0, resultLen = 0, n = 0;
		double noSpeech = 0;
		if( !readParams( f, params, nullptr ) || fscanf( f, "%d %lf %d %d", &scanFailed, &noSpeech, &resultLen, &n ) != 4 || n < 0 || resultLen > n ) rc = 2;
		else
		{
			Token* const tokens = (Token*)malloc( n ? sizeof( Token ) * (size_t)n : 1 );
			for( int i = 0; i < n && rc == 0; i++ )
			{
				double p;
				if( fscanf( f, "%d %lf", &tokens[ i ].id, &p ) != 2 ) rc = 2;
				tokens[ i ].p = (float)p;
			}
			if( rc == 0 )
			{
				fallback::Attempt a;
				a.scanFailed = scanFailed != 0;
				a.resultLen = resultLen;
				a.scores = fallback::score( tokens, resultLen );
				a.noSpeech = (float)noSpeech;
				printf( "%.17g %.17g %d %d\n", a.scores.avgLogprob, a.scores.entropy, fallback::attemptFailed( params, a ) ? 1 : 0, fallback::attemptSilent( params, a ) ? 1 : 0 );
			}
			free( tokens );
		}
	}
	else if( 0 == strcmp( argv[ 1 ], "plan" ) )
	{
		long long seek = 0;
		if( !readParams( f, params, &seek ) ) rc = 2;
		else
		{
			fallback::FallbackPlan plan( params, (int)seek );
			while( true )
			{
				int scanFailed = 0, resultLen = 0;
				double avg = 0, entropy = 0, noSpeech = 0;
				if( fscanf( f, "%d %d %lf %lf %lf", &scanFailed, &resultLen, &avg, &entropy, &noSpeech ) != 5 ) break;
				fallback::Attempt a;
				a.scanFailed = scanFailed != 0;
				a.resultLen = resultLen;
				a.scores.avgLogprob = avg;
				a.scores.entropy = entropy;
				a.noSpeech = (float)noSpeech;
				const int index = plan.attemptIndex();
				const float temperature = plan.temperature();
				const uint32_t nonce = plan.nonce();
				const int attempts = plan.attempts();
				const fallback::eVerdict v = plan.judge( a );
				printf( "%d %.9g %u %d %d\n", index, (double)temperature, nonce, attempts, (int)v );
				if( v != fallback::eVerdict::Retry ) break;
			}
		}
	}
	else rc = 1;
	fclose( f );
	if( rc ) fprintf( stderr, "bad arguments or input\n" );
	return rc;
}
