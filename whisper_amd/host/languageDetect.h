// Language "auto": the host half of whisper_lang_auto_detect (Whisper/source/whisper.cpp:2428-2495). The device half is wh_lang_detect
// (include/whisper_hip.h): the full-vocabulary softmax probabilities p of the language tokens for the window at frame 0.
// Header only: iContext::runFull (whisperImpl.cpp) and the lock-step scheduler (batchScheduler.cpp, which is also compiled into a CPU test
// library over a test double of the compute layer) share it.
#pragma once
#include "hostCommon.h"
#include <algorithm>
#include <cmath>

namespace Whisper
{
	// sFullParams::language = makeLanguageKey( "auto" ) or 0: detect (whisper_full treats nullptr, "" and "auto" alike, whisper.cpp:2789)
	constexpr uint32_t LANGUAGE_KEY_AUTO = 0x6f747561u;	  // 'a' 'u' 't' 'o' packed little-endian
	inline bool isLanguageAuto( uint32_t key ) { return key == 0 || key == LANGUAGE_KEY_AUTO; }

	// two-to-three letter code of a language id ("en"), empty when out of range
	inline std::string languageCode( int id )
	{
		const sLanguageList& list = languageList();
		std::string code;
		if( id < 0 || id >= (int)list.length ) return code;
		// the key IS the code, packed little-endian
		for( uint32_t key = list.pointer[ id ].key; key & 0xFF; key >>= 8 ) code.push_back( (char)( key & 0xFF ) );
		return code;
	}

	// Language tokens of a vocabulary: n_vocab - 51766 (99 at 51865, 100 at the large-v3 shape), none for .en models
	inline int languageTokenCount( const wh_hparams& hp ) { return hp.n_vocab >= 51865 ? hp.n_vocab - 51766 : 0; }

	// Runs for which nothing is detected because StreamRun::begin (hostLoop.h:118-135) returns before it reads the language: less than a second
	// of audio (S_FALSE), the SpeedupAudio flag (E_NOTIMPL), an audio_ctx outside the model's (E_INVALIDARG). The caller hands begin() any language
	// of the table and passes its answer on; tests hold "auto" to the answers "en" gets in these three cases.
	inline bool languageDetectionMoot( const sFullParams& params, int64_t melLen, const wh_hparams& hp )
	{
		const int seekStart = params.offset_ms / 10;
		const int seekEnd = seekStart + ( params.duration_ms == 0 ? (int)melLen : params.duration_ms / 10 );
		return seekEnd < 100 + seekStart || params.flag( eFullParamsFlags::SpeedupAudio ) || params.audio_ctx < 0 || params.audio_ctx > hp.n_audio_ctx;
	}

	// lang_probs of the reference from p[ 0 .. n ): the values sorted descending, sum = the running single-precision sum of the double exp( p ),
	// probs[ id ] = exp( p[ id ] ) / sum -- a SECOND softmax over numbers in [0, 1] (a winner with p = 0.85 comes back as ~0.023: a quirk of this
	// vintage of whisper.cpp, reproduced because it is what the reference returns). Returns the winner: the largest p, ties to the lower id.
	// probs may be nullptr.
	inline int finishLanguageProbs( const float* p, int n, float* probs )
	{
		if( !p || n <= 0 ) return -1;
		std::vector<float> sorted( p, p + n );
		std::sort( sorted.begin(), sorted.end(), []( float a, float b ) { return a > b; } );
		// whisper.cpp:2473-2481: `float sum`, and the unqualified exp() of a float resolves to the DOUBLE function under the reference's build flags:
		// every term is a double rounded into the single-precision running sum, the quotient a double rounded once (tests/test_lang_detect_cpu.py holds
		// this against the reference bit for bit; the single-precision overload does not pass)
		float sum = 0;
		for( float v : sorted ) sum += exp( (double)v );
		int best = 0;
		for( int i = 0; i < n; i++ )
		{
			if( probs ) probs[ i ] = (float)( exp( (double)p[ i ] ) / sum );
			if( p[ i ] > p[ best ] ) best = i;
		}
		return best;
	}

	// The device half as the lock-step scheduler reaches it: the signature of wh_lang_detect. batchScheduler.cpp holds NO reference to that symbol (its
	// CPU test library links against a test double of the compute layer that does not have it): whisperImpl.cpp installs &wh_lang_detect here when
	// libWhisper.so is loaded, a test library installs its own. nullptr: language "auto" in iBatchRunner::run is E_NOTIMPL.
	using pfnBatchLanguageDetector = int ( * )( wh_context* c, int batch, float* langP, int32_t* best );
	extern pfnBatchLanguageDetector g_batchLanguageDetector;
}
