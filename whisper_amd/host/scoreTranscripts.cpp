// Scoring a given transcript: Whisper::scoreTokens, scoreBatch and makeSotSequence (include/whisperApi.h) and their flat C mirror (include/whisper_c.h).
// The rules of a request are scoreRequest.h's; the device work belongs to the objects that own the device contexts (whisperImpl.cpp, batchScheduler.cpp).
#include "hostCommon.h"
#include "scoreRequest.h"
#include <cstring>

namespace Whisper
{
	namespace
	{
		// the loaded weights behind an iModel of this library (nullptr: a model of another library)
		std::shared_ptr<LoadedModel> loadedModel( iModel* model )
		{
			iModelInternals* in = nullptr;
			if( !model || FAILED( model->QueryInterface( iModelInternals::iid(), (void**)&in ) ) || !in ) return nullptr;
			std::shared_ptr<LoadedModel> lm = in->loaded();
			model->Release();	 // QueryInterface's reference
			return lm;
		}
	}

	HRESULT scoreTokens( iContext* context, const sScoreRequest& request, sTokenScore* scores )
	{
		if( !context || !scores || !request.buffer ) return E_POINTER;
		iModel* owner = nullptr;
		CHECK( context->getModel( &owner ) );
		const std::shared_ptr<LoadedModel> lm = loadedModel( owner );
		if( owner ) owner->Release();
		if( !lm )
		{
			logError( "scoreTokens: not a context of this library's createContext" );
			return E_INVALIDARG;
		}
		const score::Limits lim{ lm->hp.n_vocab, lm->vocab.token_eot, lm->vocab.token_not, lm->hp.n_text_ctx };
		int64_t n = 0;
		const float* const pcm = request.buffer->getPcmMono();
		if( !pcm ) return E_POINTER;
		HRESULT hr = score::clipRange( request.buffer->countSamples(), request.firstSample, request.countSamples, n );
		if( FAILED( hr ) )
		{
			logError( "scoreTokens: the clip must lie inside the buffer and last 1 to 30 s" );
			return hr;
		}
		score::Row row;
		hr = score::buildRow( lim, request.prompt, request.promptCount, request.tokens, request.count, request.flags, row );
		if( FAILED( hr ) )
		{
			logError( "scoreTokens: an empty prompt or token list, an id outside the vocabulary, more than %d tokens in all, or a row forced alignment cannot take", lim.maxRow() );
			return hr;
		}
		const int32_t len = (int32_t)row.tokens.size();
		std::vector<wh_token_score> recs( row.tokens.size() );
		std::vector<int32_t> frames( row.align ? row.tokens.size() : 0 );
		CHECK( contextScoreClip( context, pcm + request.firstSample, n, row.tokens.data(), len, row.firstScored, recs.data(), row.align ? frames.data() : nullptr ) );
		const std::vector<uint32_t> pass{ 0 };
		const std::vector<score::Row> rows{ row };
		score::PassArgs a;
		a.nMax = len;
		sTokenScore* const out[ 1 ] = { scores };
		score::unpackRecords( pass, rows, a, recs.data(), out );
		if( row.align )
		{
			int64_t media = 0;
			CHECK( request.buffer->getTime( media ) );
			score::alignedTimes( frames.data(), request.count, media + request.firstSample * 10000000ll / score::SAMPLE_RATE, scores );
		}
		return S_OK;
	}

	HRESULT scoreBatch( iBatchRunner* runner, const sScoreRequest* requests, uint32_t count, sTokenScore* const* scores, HRESULT* perRequest )
	{
		return runnerScore( runner, requests, count, scores, perRequest );
	}

	HRESULT makeSotSequence( iModel* model, uint32_t language, bool translate, bool timestamps, whisper_token* out, uint32_t* count )
	{
		if( !model || !count ) return E_POINTER;
		const std::shared_ptr<LoadedModel> lm = loadedModel( model );
		if( !lm )
		{
			logError( "makeSotSequence: the model was not created by this library" );
			return E_INVALIDARG;
		}
		const Vocabulary& vocab = lm->vocab;
		// the tokens that select the task, as StreamRun::begin builds them (hostLoop.h)
		std::vector<whisper_token> seq{ vocab.token_sot };
		if( vocab.isMultilingual() )
		{
			const int langId = lookupLanguageId( language );
			if( langId < 0 )
			{
				logError( "makeSotSequence: unknown language" );
				return E_INVALIDARG;
			}
			seq.push_back( vocab.token_sot + 1 + langId );
			seq.push_back( translate ? vocab.token_translate : vocab.token_transcribe );
		}
		if( !timestamps ) seq.push_back( vocab.token_not );
		const uint32_t cap = *count;
		*count = (uint32_t)seq.size();
		if( !out ) return S_OK;
		if( cap < seq.size() ) return E_BOUNDS;
		std::copy( seq.begin(), seq.end(), out );
		return S_OK;
	}
}

// ---- flat C mirror (include/whisper_c.h) ----
namespace
{
	class ClipView : public Whisper::ComObject<Whisper::iAudioBuffer>
	{
		const float* const pcm;
		const uint32_t n;
	public:
		ClipView( const float* p, uint32_t count ) : pcm( p ), n( count ) {}
		uint32_t countSamples() const override { return n; }
		const float* getPcmMono() const override { return n ? pcm : nullptr; }
		const float* getPcmStereo() const override { return nullptr; }
		HRESULT getTime( int64_t& rdi ) const override { rdi = 0; return S_OK; }
	};
	static_assert( sizeof( Whisper::sTokenScore ) == 32, "whisper_c.h documents the record as 32 bytes" );
}

extern "C" {
using namespace Whisper;

WHISPER_EXPORT int32_t whisperc_sot_sequence( void* model, const char* language, int32_t translate, int32_t timestamps, int32_t* out, uint32_t cap, uint32_t* count )
{
	if( !model || !count ) return E_POINTER;
	*count = cap;
	return makeSotSequence( (iModel*)model, makeLanguageKey( language ? language : "en" ), translate != 0, timestamps != 0, out, count );
}

WHISPER_EXPORT int32_t whisperc_score_tokens( void* ctx, const float* pcm, uint32_t nSamples, const int32_t* prompt, uint32_t promptCount, const int32_t* tokens, uint32_t count,
	uint32_t flags, void* scoresOut )
{
	if( !ctx || !pcm || !scoresOut ) return E_POINTER;
	ClipView view( pcm, nSamples );
	const sScoreRequest r{ &view, 0, 0, prompt, promptCount, tokens, count, flags };
	return scoreTokens( (iContext*)ctx, r, (sTokenScore*)scoresOut );
}

WHISPER_EXPORT int32_t whisperc_batch_score( void* runner, uint32_t count, const float* const* pcm, const uint32_t* nSamples, const int64_t* firstSample, const int64_t* countSamples,
	const int32_t* const* prompts, const uint32_t* promptCounts, const int32_t* const* tokens, const uint32_t* counts, uint32_t flags, void* const* scoresOut, int32_t* perRequest )
{
	if( !runner || ( count && ( !pcm || !nSamples || !prompts || !promptCounts || !tokens || !counts || !scoresOut ) ) ) return E_POINTER;
	std::vector<std::unique_ptr<ClipView>> views;
	std::vector<sScoreRequest> reqs( count );
	for( uint32_t i = 0; i < count; i++ )
	{
		views.emplace_back( new ClipView( pcm[ i ], nSamples[ i ] ) );
		reqs[ i ] = sScoreRequest{ views.back().get(), firstSample ? firstSample[ i ] : 0, countSamples ? countSamples[ i ] : 0, prompts[ i ], promptCounts[ i ], tokens[ i ], counts[ i ], flags };
	}
	static_assert( sizeof( HRESULT ) == sizeof( int32_t ), "perRequest is an array of HRESULT" );
	return scoreBatch( (iBatchRunner*)runner, reqs.data(), count, (sTokenScore* const*)scoresOut, (HRESULT*)perRequest );
}

}	// extern "C"
