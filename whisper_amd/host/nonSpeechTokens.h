#pragma once
// The "non-speech" tokens of a vocabulary: what openai-whisper suppresses by default (suppress_tokens = "-1") and whisper.cpp under --suppress-nst. The rule is
// whisper.cpp's, exact matches in the model's OWN vocabulary, so there is no BPE encoder here: for every symbol s of the list, every id below eot whose stored text
// is s or " " + s; and the ids whose text is " -" or " '" -- a hyphen or an apostrophe inside a word stays, one that opens a word goes. The result is ascending and
// unique. An .en or large-v3 vocabulary needs nothing special: the rule reads the file's strings.
// Host only and header only: no device symbol is named, a stand-alone driver compiles this file alone (tests/suppress_cpu/driver.cpp).
#include <algorithm>
#include <cstdint>
#include <set>
#include <string>
#include <vector>

namespace Whisper
{
	// 54 symbols, UTF-8
	inline const std::vector<std::string>& nonSpeechSymbols()
	{
		static const std::vector<std::string> symbols = {
			"\"", "#", "(", ")", "*", "+", "/", ":", ";", "<", "=", ">", "@", "[", "\\", "]", "^", "_", "`", "{", "|", "}", "~",
			"\xE3\x80\x8C", "\xE3\x80\x8D", "\xE3\x80\x8E", "\xE3\x80\x8F",								 // 「 」 『 』
			"<<", ">>", "<<<", ">>>", "--", "---", "-(", "-[", "('", "(\"", "((", "))", "(((", ")))", "[[", "]]", "{{", "}}",
			"\xE2\x99\xAA\xE2\x99\xAA", "\xE2\x99\xAA\xE2\x99\xAA\xE2\x99\xAA",							 // ♪♪ ♪♪♪
			"\xE2\x99\xA9", "\xE2\x99\xAA", "\xE2\x99\xAB", "\xE2\x99\xAC", "\xE2\x99\xAD", "\xE2\x99\xAE", "\xE2\x99\xAF",	 // ♩ ♪ ♫ ♬ ♭ ♮ ♯
		};
		return symbols;
	}

	// idToToken[ id ] = the stored text of token id; ids at or above eot (eot itself, the specials, the timestamps) are never returned
	inline std::vector<int32_t> nonSpeechTokens( const std::vector<std::string>& idToToken, int eot )
	{
		std::set<std::string> wanted;
		for( const std::string& s : nonSpeechSymbols() )
		{
			wanted.insert( s );
			wanted.insert( " " + s );
		}
		wanted.insert( " -" );
		wanted.insert( " '" );
		std::vector<int32_t> ids;
		const size_t end = eot > 0 ? std::min( (size_t)eot, idToToken.size() ) : 0;
		for( size_t id = 0; id < end; id++ )
			if( wanted.count( idToToken[ id ] ) ) ids.push_back( (int32_t)id );
		return ids;
	}
}
