// tests/score_cpu/driver.cpp -- whisper_amd/host/scoreRequest.h as a program of its own (not part of the product; built with -fsanitize=address,undefined by
// tests/test_score_cpu.py). Row building, every refusal, packing 1 / 5 / 7 requests into 1 / 2 / 5 slots and back in request order, the aligned times.
// Exit status 0 and "ok <checks>" on stdout, or the first failed check on stderr and status 1.
#include "scoreRequest.h"
#include <cstdio>
#include <cstdlib>

using namespace Whisper;

static int g_checks = 0;
#define EXPECT( cond )                                                          \
	do                                                                          \
	{                                                                           \
		g_checks++;                                                             \
		if( !( cond ) )                                                         \
		{                                                                       \
			fprintf( stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #cond ); \
			exit( 1 );                                                          \
		}                                                                       \
	} while( 0 )

// the multilingual ids: eot 50257, sot 50258, no-timestamps 50363
static const score::Limits LIM{ 51865, 50257, 50363, 448 };

static void rowsAndRefusals()
{
	const whisper_token prompt[] = { 50258, 50259, 50359, 50363 }, text[] = { 400, 401, 402 };
	score::Row row;
	EXPECT( S_OK == score::buildRow( LIM, prompt, 4, text, 3, 0, row ) );
	EXPECT( row.tokens == ( std::vector<int32_t>{ 50258, 50259, 50359, 50363, 400, 401, 402, 50257 } ) );
	EXPECT( row.firstScored == 4 && row.records() == 4 && !row.align );
	EXPECT( S_OK == score::buildRow( LIM, prompt, 4, text, 3, score::FLAG_ALIGN, row ) && row.align );
	// timestamp tokens among the scored tokens are legal without the flag, and only without it
	const whisper_token stamped[] = { 50364, 400, 50400 };
	EXPECT( S_OK == score::buildRow( LIM, prompt, 3, stamped, 3, 0, row ) && row.tokens.size() == 7 && row.firstScored == 3 );
	EXPECT( E_INVALIDARG == score::buildRow( LIM, prompt, 4, stamped, 3, score::FLAG_ALIGN, row ) );
	const whisper_token eot[] = { 400, 50257 };
	EXPECT( E_INVALIDARG == score::buildRow( LIM, prompt, 4, eot, 2, score::FLAG_ALIGN, row ) );
	// the align form: the no-timestamps token exactly once, as the prompt's last entry, behind at least one token
	EXPECT( E_INVALIDARG == score::buildRow( LIM, prompt, 3, text, 3, score::FLAG_ALIGN, row ) );
	const whisper_token twice[] = { 50258, 50363, 50359, 50363 }, early[] = { 50258, 50363, 50359 }, lone[] = { 50363 };
	EXPECT( E_INVALIDARG == score::buildRow( LIM, twice, 4, text, 3, score::FLAG_ALIGN, row ) );
	EXPECT( E_INVALIDARG == score::buildRow( LIM, early, 3, text, 3, score::FLAG_ALIGN, row ) );
	EXPECT( E_INVALIDARG == score::buildRow( LIM, lone, 1, text, 3, score::FLAG_ALIGN, row ) );
	EXPECT( S_OK == score::buildRow( LIM, twice, 4, text, 3, 0, row ) );
	// empty lists, null pointers, unknown flags, ids outside the vocabulary
	EXPECT( E_INVALIDARG == score::buildRow( LIM, prompt, 0, text, 3, 0, row ) );
	EXPECT( E_INVALIDARG == score::buildRow( LIM, prompt, 4, text, 0, 0, row ) );
	EXPECT( E_POINTER == score::buildRow( LIM, nullptr, 4, text, 3, 0, row ) && E_POINTER == score::buildRow( LIM, prompt, 4, nullptr, 3, 0, row ) );
	EXPECT( E_INVALIDARG == score::buildRow( LIM, prompt, 4, text, 3, 2, row ) );
	const whisper_token below[] = { 400, -1 }, above[] = { 51865 }, last[] = { 51864 };
	EXPECT( E_INVALIDARG == score::buildRow( LIM, prompt, 4, below, 2, 0, row ) && E_INVALIDARG == score::buildRow( LIM, prompt, 4, above, 1, 0, row ) );
	EXPECT( E_INVALIDARG == score::buildRow( LIM, below, 2, text, 3, 0, row ) && E_INVALIDARG == score::buildRow( LIM, above, 1, text, 3, 0, row ) );
	EXPECT( S_OK == score::buildRow( LIM, prompt, 4, last, 1, 0, row ) );
	// the length against the bound of wh_score_tokens: prompt + tokens + eot <= min( 256, n_text_ctx )
	std::vector<whisper_token> many( 300, 7 );
	EXPECT( S_OK == score::buildRow( LIM, prompt, 4, many.data(), 251, 0, row ) && row.tokens.size() == 256 );
	EXPECT( E_INVALIDARG == score::buildRow( LIM, prompt, 4, many.data(), 252, 0, row ) );
	const score::Limits small{ 51865, 50257, 50363, 64 };
	EXPECT( small.maxRow() == 64 && S_OK == score::buildRow( small, prompt, 4, many.data(), 59, 0, row ) && E_INVALIDARG == score::buildRow( small, prompt, 4, many.data(), 60, 0, row ) );
	// the clip: inside the buffer, 1 to 30 s
	int64_t n = -1;
	EXPECT( S_OK == score::clipRange( 480000, 0, 0, n ) && n == 480000 );
	EXPECT( S_OK == score::clipRange( 960000, 480000, 0, n ) && n == 480000 && S_OK == score::clipRange( 960000, 100, 16000, n ) && n == 16000 );
	EXPECT( E_INVALIDARG == score::clipRange( 480001, 0, 0, n ) && E_INVALIDARG == score::clipRange( 15999, 0, 0, n ) && E_INVALIDARG == score::clipRange( 960000, 0, 15999, n ) );
	EXPECT( E_INVALIDARG == score::clipRange( 960000, 900000, 100000, n ) && E_INVALIDARG == score::clipRange( 960000, -1, 16000, n ) );
	EXPECT( E_INVALIDARG == score::clipRange( 960000, 0, -5, n ) && E_INVALIDARG == score::clipRange( 960000, 960001, 0, n ) && E_INVALIDARG == score::clipRange( 0, 0, 0, n ) );
}

// `count` requests of different lengths, request `bad` (or none: -1) failing its checks, through passes of maxSlots slots and back
static void packing( uint32_t count, uint32_t maxSlots, int bad )
{
	const whisper_token prompt[] = { 50258, 50259, 50359, 50363 };
	std::vector<score::Row> rows( count );
	std::vector<HRESULT> status( count, S_OK );
	for( uint32_t r = 0; r < count; r++ )
	{
		std::vector<whisper_token> text( 2 + 3 * r );
		for( size_t k = 0; k < text.size(); k++ ) text[ k ] = (whisper_token)( 1000 * ( r + 1 ) + k );
		status[ r ] = score::buildRow( LIM, prompt, 1 + r % 4, text.data(), (int)r == bad ? 0u : (uint32_t)text.size(), 0, rows[ r ] );
		EXPECT( ( (int)r == bad ) == FAILED( status[ r ] ) );
	}
	const auto passes = score::packPasses( status, maxSlots );
	const uint32_t good = count - ( bad >= 0 ? 1 : 0 );
	EXPECT( passes.size() == ( good + maxSlots - 1 ) / maxSlots );
	std::vector<std::vector<sTokenScore>> out( count );
	std::vector<sTokenScore*> outPtr( count, nullptr );
	for( uint32_t r = 0; r < count; r++ )
	{
		out[ r ].assign( rows[ r ].tokens.empty() ? 1 : rows[ r ].records(), sTokenScore{ -7.0f, -7.0f, -7, -7, { { 77 }, { 77 } } } );
		outPtr[ r ] = out[ r ].data();
	}
	uint32_t next = 0;
	for( const auto& pass : passes )
	{
		EXPECT( !pass.empty() && pass.size() <= maxSlots );
		for( uint32_t r : pass )
		{
			// request order, the failing request left out
			if( (int)next == bad ) next++;
			EXPECT( r == next );
			next++;
		}
		const score::PassArgs a = score::packTokens( pass, rows );
		EXPECT( a.lens.size() == pass.size() && a.first.size() == pass.size() && a.tokens.size() == pass.size() * (size_t)a.nMax );
		// what the device would answer: a record that names its slot and entry; entries that are not scored stay zero
		std::vector<wh_token_score> recs( a.tokens.size(), wh_token_score{ 0, 0, 0, 0 } );
		for( size_t s = 0; s < pass.size(); s++ )
		{
			const score::Row& row = rows[ pass[ s ] ];
			EXPECT( a.lens[ s ] == (int32_t)row.tokens.size() && a.first[ s ] == row.firstScored && a.lens[ s ] <= a.nMax );
			for( int i = 0; i < a.nMax; i++ )
			{
				const int32_t t = a.tokens[ s * (size_t)a.nMax + (size_t)i ];
				EXPECT( t == ( i < a.lens[ s ] ? row.tokens[ (size_t)i ] : 0 ) );
				if( i >= a.first[ s ] && i < a.lens[ s ] ) recs[ s * (size_t)a.nMax + (size_t)i ] = wh_token_score{ -(float)t, -0.5f, t, i };
			}
		}
		score::unpackRecords( pass, rows, a, recs.data(), outPtr.data() );
	}
	for( uint32_t r = 0; r < count; r++ )
	{
		if( (int)r == bad )
		{
			EXPECT( out[ r ][ 0 ].rank == -7 );	   // a request that failed its checks is never written
			continue;
		}
		const score::Row& row = rows[ r ];
		for( uint32_t k = 0; k < row.records(); k++ )
		{
			const sTokenScore& s = out[ r ][ k ];
			const int32_t t = row.tokens[ (size_t)row.firstScored + k ];
			EXPECT( s.best == t && s.logprob == -(float)t && s.rank == row.firstScored + (int32_t)k && s.bestLogprob == -0.5f && s.time.begin.ticks == 0 && s.time.end.ticks == 0 );
		}
		EXPECT( out[ r ][ row.records() - 1 ].best == LIM.tokenEot );
	}
}

static void times()
{
	// three text tokens at 20 ms positions 5, 9, 9 and the end of the text at 40: a text token lasts to the next one's start, eot sits at the end
	const int32_t frames[] = { 5, 9, 9, 40 };
	sTokenScore s[ 4 ] = {};
	score::alignedTimes( frames, 3, 1234, s );
	const uint64_t want[ 4 ][ 2 ] = { { 1000000, 1800000 }, { 1800000, 1800000 }, { 1800000, 8000000 }, { 8000000, 8000000 } };
	for( int k = 0; k < 4; k++ ) EXPECT( s[ k ].time.begin.ticks == want[ k ][ 0 ] + 1234 && s[ k ].time.end.ticks == want[ k ][ 1 ] + 1234 );
}

int main()
{
	rowsAndRefusals();
	const uint32_t counts[] = { 1, 5, 7 }, slots[] = { 1, 2, 5 };
	for( uint32_t c : counts )
		for( uint32_t m : slots )
		{
			packing( c, m, -1 );
			packing( c, m, (int)( c / 2 ) );
		}
	EXPECT( score::packPasses( {}, 4 ).empty() && score::packPasses( { E_INVALIDARG, E_POINTER }, 4 ).empty() );
	times();
	printf( "ok %d\n", g_checks );
	return 0;
}
