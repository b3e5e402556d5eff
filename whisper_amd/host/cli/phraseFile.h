#pragma once
// --boost-phrases FILE of whisper-main and whisper-mgpu: a UTF-8 file, one phrase per line, blank lines ignored; every phrase gives its spellings
// (Whisper::phraseSpellings) and all of them become the rows of one sBoostedPhrases. Header only, over whisperApi.h.
#include "whisperApi.h"
#include <cstdint>
#include <fstream>
#include <string>
#include <vector>

namespace phraseFile
{
	struct Rows
	{
		std::vector<int32_t> tokens, lengths;	  // [ count ][ 16 ], [ count ]
		Whisper::sBoostedPhrases set( float boost ) const { return Whisper::sBoostedPhrases{ tokens.data(), lengths.data(), (uint32_t)lengths.size(), 16, boost }; }
	};

	// S_OK, or the failure with `why` saying what to print
	inline HRESULT load( Whisper::iModel* model, const std::string& path, Rows& rows, std::string& why )
	{
		std::ifstream f( path, std::ios::binary );
		if( !f ) { why = "cannot open the phrase file '" + path + "'"; return E_INVALIDARG; }
		std::string line;
		bool first = true;
		while( std::getline( f, line ) )
		{
			if( first && line.size() >= 3 && !line.compare( 0, 3, "\xEF\xBB\xBF" ) ) line.erase( 0, 3 );	 // a byte-order mark
			first = false;
			while( !line.empty() && ( line.back() == '\r' || line.back() == '\n' || line.back() == ' ' || line.back() == '\t' ) ) line.pop_back();
			if( line.find_first_not_of( " \t" ) == std::string::npos ) continue;
			int32_t tokens[ 2 * 16 ], lengths[ 2 ];
			uint32_t n = 2;
			const HRESULT hr = Whisper::phraseSpellings( model, line.c_str(), tokens, lengths, &n );
			if( FAILED( hr ) ) { why = "the phrase '" + line + "' of '" + path + "' cannot be boosted (1 .. 16 tokens)"; return hr; }
			for( uint32_t r = 0; r < n; r++ )
			{
				rows.tokens.insert( rows.tokens.end(), tokens + 16 * r, tokens + 16 * r + 16 );
				rows.lengths.push_back( lengths[ r ] );
			}
		}
		if( rows.lengths.empty() ) { why = "the phrase file '" + path + "' holds no phrase"; return E_INVALIDARG; }
		return S_OK;
	}
}
