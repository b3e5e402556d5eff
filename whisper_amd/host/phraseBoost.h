#pragma once
// Phrase boosting on the host ("Phrase boosting"): the checks Whisper::setBoostedPhrases and setBatchBoostedPhrases share, and the two
// spellings of a text phrase. Host only and header only: no device symbol is named, so the scheduler's CPU test library compiles it as it is.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace Whisper
{
	namespace phraseBoost
	{
		// the limits of one set (wh_context_set_boost states them for the device; the table-entry cap is the compiler's to check)
		constexpr uint32_t MAX_PHRASES = 1024, MAX_LENGTH = 16;

		// A checked copy of a caller's set, rows `nMax` apart as wh_context_set_boost takes them; count == 0 = no set
		struct Set
		{
			std::vector<int32_t> tokens, lens;
			int nMax = 0;
			float boost = 0.0f;
			int count() const { return (int)lens.size(); }
		};

		// nullptr when the set is fine, else the sentence for the log. tokens [count][maxLength], lengths [count]
		inline const char* check( const int32_t* tokens, const int32_t* lengths, uint32_t count, uint32_t maxLength, float boost, int tokenEot, Set& out, std::string& text )
		{
			out = Set{};
			if( count == 0 ) return nullptr;
			if( !tokens || !lengths ) return "null tokens or lengths";
			char buf[ 160 ];
			if( count > MAX_PHRASES )
			{
				snprintf( buf, sizeof( buf ), "%u phrases, the limit is %u", count, MAX_PHRASES );
				return ( text = buf ).c_str();
			}
			if( !std::isfinite( boost ) || !( boost > 0.0f ) ) return "the boost must be finite and greater than 0";
			for( uint32_t p = 0; p < count; p++ )
			{
				if( lengths[ p ] < 1 || (uint32_t)lengths[ p ] > MAX_LENGTH || (uint32_t)lengths[ p ] > maxLength )
				{
					snprintf( buf, sizeof( buf ), "phrase %u has %i tokens, a phrase has 1 .. %u", p, (int)lengths[ p ], MAX_LENGTH );
					return ( text = buf ).c_str();
				}
				for( int i = 0; i < lengths[ p ]; i++ )
				{
					const int32_t t = tokens[ (size_t)p * maxLength + i ];
					if( t >= 0 && t < tokenEot ) continue;
					snprintf( buf, sizeof( buf ), "id %i of phrase %u is outside [ 0, %i ): only text tokens can be boosted", (int)t, p, tokenEot );
					return ( text = buf ).c_str();
				}
			}
			out.tokens.assign( tokens, tokens + (size_t)count * maxLength );
			out.lens.assign( lengths, lengths + count );
			out.nMax = (int)maxLength;
			out.boost = boost;
			return nullptr;
		}

		// The spellings of one text phrase as token rows: the text as written and, when it does not begin with a space, the text behind one space -- how a word is
		// spelled in mid-sentence. `tokenize` is the model's ( const char*, std::vector<int>& ) -> bool. Rows that come out equal collapse. false: a row is empty
		// or longer than MAX_LENGTH, `text` then names the phrase
		template<class Tokenize>
		inline bool spellings( const char* phrase, Tokenize&& tokenize, std::vector<std::vector<int>>& rows, std::string& text )
		{
			rows.clear();
			const std::string written = phrase ? phrase : "";
			std::vector<std::string> forms{ written };
			if( written.empty() || written[ 0 ] != ' ' ) forms.push_back( " " + written );
			for( const std::string& f : forms )
			{
				std::vector<int> row;
				const bool ok = !written.empty() && tokenize( f.c_str(), row );
				if( !ok || row.empty() || row.size() > MAX_LENGTH )
				{
					text = "the phrase \"" + written + "\" gives " + std::to_string( row.size() ) + " tokens, a phrase has 1 .. 16";
					rows.clear();
					return false;
				}
				bool seen = false;
				for( const auto& r : rows ) seen = seen || r == row;
				if( !seen ) rows.push_back( row );
			}
			return true;
		}
	}
}
