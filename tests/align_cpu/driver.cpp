// tests/align_cpu/driver.cpp -- a CPU test harness for the AlignTokens half of the host loop (not part of the product, never shipped).
// whisper_amd/host/hostLoop.h's StreamRun and WindowScan with a SCRIPTED aligner and scripted tokens: what is under test is how a window's
// frames become token times (text tokens, timestamp tokens, other specials, two segments in a window, max_len wrapping), that the aligner is
// asked once per window with the window's own sot sequence, text, seek and end -- and never without the flag. Built by tests/test_align_cpu.py.
//
//   driver <flags> <max_len> <mel_len> <with_pcm> <window> ...      window = "id,id,...;frame,frame,..."
// Prints {"hr":..,"segments":[{"t0","t1","text","tokens":[{"id","t0","t1","vlen"}]}],"calls":[{"seek","seekEnd","sot":[..],"text":[..]}],"new_segments":n}
#include "hostLoop.h"
#include <cstdio>
#include <cstdlib>
#include <sstream>

namespace Whisper
{
	eHostLoopRules g_hostLoopRules = eHostLoopRules::ReferenceCpu;
}
using namespace Whisper;

namespace
{
	std::vector<int> numbers( const std::string& s )
	{
		std::vector<int> out;
		std::istringstream in( s );
		std::string item;
		while( std::getline( in, item, ',' ) )
			if( !item.empty() ) out.push_back( atoi( item.c_str() ) );
		return out;
	}
	struct Call { int seek, seekEnd; std::vector<int> sot, text; };
	struct ScriptedAligner : iTokenAligner
	{
		std::vector<std::vector<int>> frames;	  // per window
		std::vector<Call> calls;
		HRESULT alignWindow( int seek, int seekEnd, const std::vector<int>& sotSequence, const std::vector<int>& text, std::vector<int>& out ) override
		{
			if( calls.size() >= frames.size() ) return E_FAIL;
			out = frames[ calls.size() ];
			calls.push_back( Call{ seek, seekEnd, sotSequence, text } );
			return S_OK;
		}
	};
	int g_newSegments = 0;
	HRESULT newSegment( iContext*, uint32_t nNew, void* ) noexcept { g_newSegments += (int)nNew; return S_OK; }
	void list( std::ostringstream& o, const std::vector<int>& v )
	{
		o << "[";
		for( size_t i = 0; i < v.size(); i++ ) o << ( i ? "," : "" ) << v[ i ];
		o << "]";
	}
}

int main( int argc, char** argv )
{
	if( argc < 6 ) return 2;
	const uint32_t flags = (uint32_t)strtoul( argv[ 1 ], nullptr, 0 );
	const int maxLen = atoi( argv[ 2 ] ), melLen = atoi( argv[ 3 ] ), withPcm = atoi( argv[ 4 ] );

	// a multilingual vocabulary whose text tokens are the words " w<id>"
	Vocabulary vocab;
	vocab.idToToken.resize( 50257 );
	for( int i = 0; i < 50257; i++ ) vocab.idToToken[ (size_t)i ] = " w" + std::to_string( i );
	vocab.idToToken[ 99 ].clear();	   // a text token that prints nothing: a range holding only such tokens is not emitted as a segment
	vocab.finalize( 51865 );
	const wh_hparams hp{ 51865, 1500, 128, 2, 4, 448, 128, 2, 4, 80, 1 };

	sFullParams p{};
	p.strategy = eSamplingStrategy::Greedy;
	p.n_max_text_ctx = 16384;
	p.flags = (eFullParamsFlags)flags;
	p.language = makeLanguageKey( "en" );
	p.thold_pt = p.thold_ptsum = 0.01f;
	p.max_len = maxLen;
	p.new_segment_callback = &newSegment;

	ScriptedAligner aligner;
	std::vector<std::vector<int>> windows;
	for( int i = 5; i < argc; i++ )
	{
		const std::string w = argv[ i ];
		const size_t semi = w.find( ';' );
		windows.push_back( numbers( w.substr( 0, semi ) ) );
		aligner.frames.push_back( semi == std::string::npos ? std::vector<int>() : numbers( w.substr( semi + 1 ) ) );
	}

	std::vector<Segment> resultAll;
	std::vector<int> promptPast;
	TokenTimestamper stamper;
	std::vector<float> pcm;
	if( withPcm )
	{
		pcm.resize( (size_t)melLen * 160 );
		for( size_t i = 0; i < pcm.size(); i++ ) pcm[ i ] = 0.1f * (float)( ( i * 7919 ) % 200 ) / 200.0f - 0.05f;
		stamper.begin( pcm.data(), pcm.size() );
	}
	const sProgressSink sink{ nullptr, nullptr };
	StreamRun run( p, vocab, hp, nullptr, sink, resultAll, promptPast, &stamper );
	run.setAligner( &aligner );
	HRESULT hr = run.begin( melLen );
	size_t next = 0;
	if( hr == S_OK )
	{
		std::vector<int> prompt;
		while( true )
		{
			hr = run.nextWindow( prompt );
			if( hr != S_OK || next >= windows.size() ) break;
			WindowScan scan( run.fullParams(), vocab, run.seek, run.seekEnd(), run.maxTokens() );
			for( int id : windows[ next ] )
			{
				TokenData t;
				t.id = id;
				t.tid = id > vocab.token_beg ? id : vocab.token_beg;
				t.p = t.pt = t.ptsum = 0.5f;
				if( scan.feed( t ) ) break;
			}
			next++;
			hr = run.finishWindow( scan );
			if( FAILED( hr ) ) break;
		}
		if( hr == S_FALSE ) hr = run.end();
	}

	std::ostringstream o;
	o.precision( 9 );
	o << "{\"hr\":" << hr << ",\"segments\":[";
	for( size_t i = 0; i < resultAll.size(); i++ )
	{
		const Segment& s = resultAll[ i ];
		o << ( i ? "," : "" ) << "{\"t0\":" << s.t0 << ",\"t1\":" << s.t1 << ",\"text\":\"" << s.text << "\",\"tokens\":[";
		for( size_t j = 0; j < s.tokens.size(); j++ )
		{
			const TokenData& t = s.tokens[ j ];
			o << ( j ? "," : "" ) << "{\"id\":" << t.id << ",\"t0\":" << t.t0 << ",\"t1\":" << t.t1 << ",\"vlen\":" << t.vlen << "}";
		}
		o << "]}";
	}
	o << "],\"calls\":[";
	for( size_t i = 0; i < aligner.calls.size(); i++ )
	{
		const Call& c = aligner.calls[ i ];
		o << ( i ? "," : "" ) << "{\"seek\":" << c.seek << ",\"seekEnd\":" << c.seekEnd << ",\"sot\":";
		list( o, c.sot );
		o << ",\"text\":";
		list( o, c.text );
		o << "}";
	}
	o << "],\"new_segments\":" << g_newSegments << "}";
	puts( o.str().c_str() );
	return 0;
}
