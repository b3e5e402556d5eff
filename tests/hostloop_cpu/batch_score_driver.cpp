// tests/hostloop_cpu/batch_score_driver.cpp -- CPU test harness for Whisper::scoreBatch in the lock-step batch scheduler (not part of the product).
// One translation unit = the test double of the compute layer (fake_device.cpp) and the batch harness (batch_driver.cpp), both UNCHANGED, plus
//   * the scorer the scheduler gets injected (scoreRequest.h g_batchScorer): wh_score_tokens played by the double's per-slot reference models -- the row through
//     whisper_decode at position 0, the records of the definition (DESIGN.md section 7 "Scoring") from the logits of every fed row, in double;
//   * bs_run: requests over buffers through createBatchRunner + the scheduler's scoring entry, the records and per-request results as JSON.
#include "fake_device.cpp"
#include "batch_driver.cpp"
#include "scoreRequest.h"
#include <cmath>

extern "C" {
size_t ref_logits_size( void* ctx );
void ref_get_logits( void* ctx, float* dst );
}

namespace
{
	std::vector<int> g_scoreCalls;	   // windows of every call of the scorer
	int fakeScoreTokens( wh_context* c, int batch, const int32_t* tokens, const int32_t* lens, const int32_t* firstScored, int nMax, wh_token_score* out )
	{
		if( !c || batch != c->batch || !tokens || !lens || !firstScored || !out ) return WH_E_INVALIDARG;
		g_scoreCalls.push_back( batch );
		memset( out, 0, sizeof( wh_token_score ) * (size_t)batch * (size_t)nMax );
		for( int b = 0; b < batch; b++ )
		{
			if( !c->active[ b ] || lens[ b ] < 2 || lens[ b ] > nMax || firstScored[ b ] < 1 || firstScored[ b ] >= lens[ b ] ) return WH_E_INVALIDARG;
			void* w = c->cpu[ b ];
			int32_t hp[ 11 ];
			ref_hparams( w, hp );
			const int nVocab = hp[ 0 ];
			const int32_t* row = tokens + (size_t)b * nMax;
			if( 0 != ref_decode( w, row, lens[ b ], 0, c->model->threads ) ) return -1;
			std::vector<float> logits( ref_logits_size( w ) );
			if( logits.size() != (size_t)lens[ b ] * nVocab ) return -1;
			ref_get_logits( w, logits.data() );
			for( int i = firstScored[ b ]; i < lens[ b ]; i++ )
			{
				const float* x = logits.data() + (size_t)( i - 1 ) * nVocab;
				const int t = row[ i ];
				float m = -INFINITY;
				int best = 0;
				for( int j = 0; j < nVocab; j++ )
					if( x[ j ] > m ) { m = x[ j ]; best = j; }
				double s = 0.0;
				int rank = 0;
				for( int j = 0; j < nVocab; j++ )
				{
					if( x[ j ] != -INFINITY ) s += exp( (double)x[ j ] - (double)m );
					if( x[ j ] > x[ t ] || ( x[ j ] == x[ t ] && j < t ) ) rank++;
				}
				out[ (size_t)b * nMax + i ] = wh_token_score{ (float)( (double)x[ t ] - (double)m - log( s ) ), (float)( -log( s ) ), best, rank };
			}
		}
		return 0;
	}
	const bool g_scorerInstalled = ( Whisper::g_batchScorer = &fakeScoreTokens, true );
	std::string g_scoreOut;
}

// install = 0: the scheduler without a scorer (scoreBatch must be E_NOTIMPL)
extern "C" __attribute__( ( visibility( "default" ) ) ) void bs_install_scorer( int install ) { Whisper::g_batchScorer = install ? &fakeScoreTokens : nullptr; }

struct ScoreRequestDesc
{
	int32_t buffer;					  // index into the buffers of the call
	int32_t promptOff, promptCount, tokenOff, tokenCount;	  // into the token pool
	uint32_t flags;
	int64_t firstSample, countSamples;
};

// bs_result() = {"hr":..,"calls":[windows per call of the scorer],"requests":[{"hr":..,"records":[[logprob,bestLogprob,best,rank],..]}]}
extern "C" __attribute__( ( visibility( "default" ) ) ) int bs_run( const char* modelPath, const float* const* pcm, const int32_t* nSamples, int nBuffers,
	const ScoreRequestDesc* reqs, int nReqs, const int32_t* pool, uint32_t maxSlots, int threads )
{
	g_scoreOut.clear();
	g_scoreCalls.clear();
	std::shared_ptr<LoadedModel> lm = std::make_shared<LoadedModel>();
	HRESULT hr = loadVocabulary( modelPath, lm->vocab );
	if( FAILED( hr ) ) return hr;
	{
		void* w = ref_init( modelPath );
		if( !w ) return E_FAIL;
		int32_t h[ 11 ];
		ref_hparams( w, h );
		ref_free( w );
		lm->hp = wh_hparams{ h[ 0 ], h[ 1 ], h[ 2 ], h[ 3 ], h[ 4 ], h[ 5 ], h[ 6 ], h[ 7 ], h[ 8 ], h[ 9 ], h[ 10 ] };
	}
	lm->gpu = fake_model_create( modelPath, threads );
	TestModel model( lm );
	std::vector<MemoryBuffer> buffers( (size_t)nBuffers );
	for( int b = 0; b < nBuffers; b++ ) buffers[ b ].pcm.assign( pcm[ b ], pcm[ b ] + nSamples[ b ] );
	std::vector<sScoreRequest> requests( (size_t)nReqs );
	std::vector<std::vector<sTokenScore>> scores( (size_t)nReqs );
	std::vector<sTokenScore*> scorePtr( (size_t)nReqs );
	for( int i = 0; i < nReqs; i++ )
	{
		const ScoreRequestDesc& d = reqs[ i ];
		requests[ i ] = sScoreRequest{ d.buffer >= 0 ? &buffers[ d.buffer ] : nullptr, d.firstSample, d.countSamples, pool + d.promptOff, (uint32_t)d.promptCount,
			pool + d.tokenOff, (uint32_t)d.tokenCount, d.flags };
		scores[ i ].assign( (size_t)d.tokenCount + 1, sTokenScore{ -7.0f, -7.0f, -7, -7, { { 7 }, { 7 } } } );
		scorePtr[ i ] = scores[ i ].data();
	}
	const sBatchSetup setup{ maxSlots, 1, 4, 0 };
	iBatchRunner* runner = nullptr;
	hr = createBatchRunner( &model, &setup, &runner );
	if( FAILED( hr ) ) return hr;
	std::vector<HRESULT> per( (size_t)nReqs, S_OK );
	hr = runnerScore( runner, requests.data(), (uint32_t)nReqs, scorePtr.data(), per.data() );
	std::ostringstream o;
	o.precision( 9 );
	o << "{\"hr\":" << hr << ",\"calls\":[";
	for( size_t i = 0; i < g_scoreCalls.size(); i++ ) o << ( i ? "," : "" ) << g_scoreCalls[ i ];
	o << "],\"requests\":[";
	for( int i = 0; i < nReqs; i++ )
	{
		o << ( i ? "," : "" ) << "{\"hr\":" << per[ i ] << ",\"records\":[";
		for( size_t k = 0; k < scores[ i ].size(); k++ )
		{
			const sTokenScore& s = scores[ i ][ k ];
			o << ( k ? "," : "" ) << "[" << s.logprob << "," << s.bestLogprob << "," << s.best << "," << s.rank << "," << s.time.begin.ticks << "]";
		}
		o << "]}";
	}
	o << "]}";
	g_scoreOut = o.str();
	runner->Release();
	return hr;
}
extern "C" __attribute__( ( visibility( "default" ) ) ) const char* bs_result() { return g_scoreOut.c_str(); }
