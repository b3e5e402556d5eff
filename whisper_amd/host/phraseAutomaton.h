#pragma once
// --allow-phrases FILE of whisper-main and whisper-mgpu: the byte-level automaton of a phrase list for Whisper::setDecodingConstraint (DESIGN.md section 7,
// "Constrained decoding"). THE SAME RULE AS api.compile_phrases of whisper_amd/api.py, AND THE TWO MUST AGREE, state for state: a trie over the phrases' UTF-8
// bytes in the order given; one space may come first (or must, or must not); under `repeat` one space leads from a phrase's end to the next phrase; made
// deterministic by the subset construction, the subsets numbered in the order a breadth-first walk over the ascending used bytes meets them; the bytes no phrase
// uses share the last class, which has no transitions. tests/test_gpu_constraint_library.py compares the two through the transcript.
// Header only, over whisperApi.h.
#include "whisperApi.h"
#include <cstdint>
#include <fstream>
#include <map>
#include <set>
#include <string>
#include <vector>

namespace phraseAutomaton
{
	enum struct eLeadingSpace { Optional, Always, Never };

	struct Dfa
	{
		std::vector<uint8_t> classOf, accept;	  // [ 256 ], [ states ]
		std::vector<int32_t> trans;				  // [ states ][ classes ]
		uint32_t states = 0, classes = 0;
		Whisper::sDecodingConstraint constraint( float penalty ) const
		{
			return Whisper::sDecodingConstraint{ states, classes, 0, classOf.data(), trans.data(), accept.data(), penalty };
		}
	};

	// false with `why` for an empty list or an empty phrase
	inline bool compile( const std::vector<std::string>& phrases, eLeadingSpace lead, bool repeat, Dfa& dfa, std::string& why )
	{
		std::vector<std::map<int, int>> kids( 1 );	 // the trie: node 0 is its root
		std::set<int> ends;
		for( const std::string& p : phrases )
		{
			if( p.empty() ) { why = "an empty phrase"; return false; }
			int n = 0;
			for( const char ch : p )
			{
				const int b = (uint8_t)ch;
				const auto it = kids[ (size_t)n ].find( b );
				if( it != kids[ (size_t)n ].end() ) { n = it->second; continue; }
				const int fresh = (int)kids.size();
				kids[ (size_t)n ][ b ] = fresh;
				kids.emplace_back();
				n = fresh;
			}
			ends.insert( n );
		}
		if( kids.size() == 1 ) { why = "no phrases"; return false; }
		constexpr int START = -1;	// in front of the optional space
		const auto step = [ & ]( const std::set<int>& subset, int b )
		{
			std::set<int> out;
			for( const int n : subset )
			{
				if( n == START )
				{
					if( b == 32 && lead != eLeadingSpace::Never ) out.insert( 0 );
					if( lead != eLeadingSpace::Always && kids[ 0 ].count( b ) ) out.insert( kids[ 0 ].at( b ) );
					continue;
				}
				const auto it = kids[ (size_t)n ].find( b );
				if( it != kids[ (size_t)n ].end() ) out.insert( it->second );
				if( repeat && b == 32 && ends.count( n ) ) out.insert( 0 );
			}
			return out;
		};
		std::set<int> usedSet{ 32 };
		for( const auto& k : kids )
			for( const auto& kv : k ) usedSet.insert( kv.first );
		const std::vector<int> used( usedSet.begin(), usedSet.end() );
		dfa = Dfa{};
		dfa.classes = (uint32_t)used.size() + 1;
		dfa.classOf.assign( 256, (uint8_t)used.size() );
		for( size_t c = 0; c < used.size(); c++ ) dfa.classOf[ (size_t)used[ c ] ] = (uint8_t)c;
		std::map<std::set<int>, int> index;
		std::vector<std::set<int>> order{ std::set<int>{ START } };
		index[ order[ 0 ] ] = 0;
		for( size_t s = 0; s < order.size(); s++ )	 // grows while it is walked
		{
			const std::set<int> subset = order[ s ];
			std::vector<int32_t> row( dfa.classes, -1 );
			for( size_t c = 0; c < used.size(); c++ )
			{
				const std::set<int> next = step( subset, used[ c ] );
				if( next.empty() ) continue;
				const auto found = index.find( next );
				if( found != index.end() ) { row[ c ] = found->second; continue; }
				row[ c ] = (int32_t)order.size();
				index[ next ] = (int)order.size();
				order.push_back( next );
			}
			dfa.trans.insert( dfa.trans.end(), row.begin(), row.end() );
		}
		dfa.states = (uint32_t)order.size();
		for( const std::set<int>& subset : order )
		{
			bool acc = false;
			for( const int n : subset ) acc = acc || ends.count( n ) != 0;
			dfa.accept.push_back( acc ? 1 : 0 );
		}
		return true;
	}

	// the file of --allow-phrases: UTF-8, one phrase per line, a byte-order mark, trailing blanks and blank lines ignored (phraseFile.h reads --boost-phrases so)
	inline HRESULT load( const std::string& path, eLeadingSpace lead, bool repeat, Dfa& dfa, std::string& why )
	{
		std::ifstream f( path, std::ios::binary );
		if( !f ) { why = "cannot open the phrase file '" + path + "'"; return E_INVALIDARG; }
		std::vector<std::string> phrases;
		std::string line;
		bool first = true;
		while( std::getline( f, line ) )
		{
			if( first && line.size() >= 3 && !line.compare( 0, 3, "\xEF\xBB\xBF" ) ) line.erase( 0, 3 );
			first = false;
			while( !line.empty() && ( line.back() == '\r' || line.back() == '\n' || line.back() == ' ' || line.back() == '\t' ) ) line.pop_back();
			if( line.find_first_not_of( " \t" ) == std::string::npos ) continue;
			phrases.push_back( line );
		}
		if( compile( phrases, lead, repeat, dfa, why ) ) return S_OK;
		why = "the phrase file '" + path + "': " + why;
		return E_INVALIDARG;
	}
}
