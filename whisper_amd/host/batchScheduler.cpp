// Whisper::runFullBatch -- K streams in lock step behind the drop-in boundary (extension next to loadModelShared).
//
// The reference transcribes one recording per iContext, window after window (ContextImpl::runFullImpl, Whisper/Whisper/ContextImpl.cpp:
// 452-793); its only multi-instance facilities are whisper_full_parallel (Whisper/source/whisper.cpp:3127: n processors, each a slice of
// the recording) and iModel::clone + a context per thread (Whisper/Whisper/ModelImpl.cpp:40-60). On MI355X a decode step of ONE sequence
// is a chain of ~200 launches at their latency floors that leaves the chip idle; the same chain carries 64 or 112 sequences for about
// the same time. So the streams' NEXT windows are made one encoder batch and one decode chain:
//
//   group   = one wh_context of `slots` windows (own HIP stream, own captured decode graph, own KV caches)
//   slot    = the stream currently assigned to a row of the group's batch; a finished stream's slot takes the next pending stream
//   round   = every slot's next window: StreamRun::nextWindow (progress / encoder_begin callbacks, prompt with the stream's own past
//             text) -> wh_encode_windows (each slot its own spectrogram and seek) -> wh_decode_window_start_ragged (prompts of
//             different lengths, a position per sequence) -> greedy chunks, scanned chunk by chunk with WindowScan until every slot's
//             window is over -> StreamRun::finishWindow per slot (segments, callbacks, seek += the stream's own delta)
//   retry   = with Whisper::setBatchDecodingFallback on, a window whose attempt fails its gates STAYS in its slot -- same seek, same prompt, no nextWindow
//             and no finishWindow -- and is decoded again in the next round at the plan's next temperature while its neighbours move on: a retried window
//             costs one slot-round (the round encodes every slot anyway). The rows of a round sample each under its own temperature, key and nonce.
//
// Rounds of different groups overlap on the GPU (the MFMA-bound encoder of one under the latency-bound decode chain of the other);
// ONE host thread -- the caller's, so callbacks arrive on the calling thread like runFull's -- serves all groups through
// wh_decode_window_ready polls. Per stream the rules are hostLoop.h's, the same objects iContext::runFull uses: a stream's transcript
// is the transcript of runFull on the same samples (tests/test_batch_api.py).
#include "hostCommon.h"
#include "hostLoop.h"
#include "batchSampling.h"
#include "batchSuppress.h"
#include "batchTimestampRules.h"
#include "batchBoost.h"
#include "batchNoRepeat.h"
#include "batchSpeech.h"
#include "optionRules.h"
#include "decodeFallback.h"
#include "languageDetect.h"
#include "scoreRequest.h"
#include "results.h"
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <thread>

namespace Whisper
{
	// The device half of language detection, injected (languageDetect.h): this file names no entry point of the compute layer for it
	pfnBatchLanguageDetector g_batchLanguageDetector = nullptr;
	// ... and for per-row sampling and the no-speech gather (batchSampling.h)
	const BatchSamplingHooks* g_batchSamplingHooks = nullptr;
	// ... and for suppressed tokens (batchSuppress.h)
	pfnBatchSuppress g_batchSuppress = nullptr;
	// ... and for the timestamp rules (batchTimestampRules.h)
	pfnBatchTimestampRules g_batchTimestampRules = nullptr;
	// ... and for boosted phrases (batchBoost.h)
	pfnBatchBoost g_batchBoost = nullptr;
	// ... and for no-repeat n-grams (batchNoRepeat.h)
	pfnBatchNoRepeat g_batchNoRepeat = nullptr;
	// ... and to the scorer of given transcripts (scoreRequest.h)
	pfnBatchScorer g_batchScorer = nullptr;
	// ... and to the speech filter of a newly admitted stream (batchSpeech.h)
	pfnBatchSpeechPacker g_batchSpeechPacker = nullptr;

	namespace
	{
		// What a stream's callbacks receive: results so far and the model; running anything through it is not possible.
		class StreamContext : public ComObject<iContext>
		{
			iModel* const owner;
			const Vocabulary& vocab;
			// what getResults hands out without NewObject: embedded, Release never deletes -- the ownership ContextImpl has
			// (a heap object held in a raw pointer here was freed by the first callback that released it the reference's way)
			mutable TranscribeResultStatic live;
		public:
			std::vector<Segment> resultAll;
			int64_t mediaTimeOffset = 0;
			// detectSpeaker (diarize.h): the stream's piece of its buffer's stereo PCM -- getPcmStereo() advanced by 2 * firstSample, the stream's
			// countSamples frames of it -- or nullptr. mediaTimeOffset already accounts for firstSample. The context exists only while its stream runs.
			const float* stereoPcm = nullptr;
			size_t stereoFrames = 0;
			mutable std::vector<uint8_t> speakers;	   // per segment of resultAll
			void labelNewSegments() const { appendSpeakers( resultAll, mediaTimeOffset, stereoPcm, stereoFrames, speakers ); }
			StreamContext( iModel* m, const Vocabulary& v ) : owner( m ), vocab( v ) {}
			HRESULT runFull( const sFullParams&, const iAudioBuffer* ) override { return E_NOTIMPL; }
			HRESULT runStreamed( const sFullParams&, const sProgressSink&, const iAudioReader* ) override { return E_NOTIMPL; }
			HRESULT runCapture( const sFullParams&, const sCaptureCallbacks&, const iAudioCapture* ) override { return E_NOTIMPL; }
			HRESULT getResults( eResultFlags flags, iTranscribeResult** pp ) const override
			{
				if( !pp ) return E_POINTER;
				labelNewSegments();	   // a segment whose new_segment callback is running
				if( flags & eResultFlags::NewObject )
				{
					TranscribeResult* r = new TranscribeResult();
					r->speakers = speakers;
					const HRESULT hr = fillResultData( resultAll, vocab, mediaTimeOffset, flags, *r );
					if( FAILED( hr ) ) { r->Release(); return hr; }
					*pp = r;
					return S_OK;
				}
				// without NewObject the reference hands out an object that lives as long as the context (TranscribeResult.h:34-43)
				live.speakers = speakers;
				CHECK( fillResultData( resultAll, vocab, mediaTimeOffset, flags, live ) );
				*pp = &live;
				return S_OK;
			}
			HRESULT detectSpeaker( const sTimeInterval& time, eSpeakerChannel& result ) const override
			{
				return diarize::detectSpeaker( stereoPcm, stereoFrames, mediaTimeOffset, time, result );
			}
			HRESULT getModel( iModel** pp ) override
			{
				if( !pp ) return E_POINTER;
				owner->AddRef();
				*pp = owner;
				return S_OK;
			}
			HRESULT fullDefaultParams( eSamplingStrategy, sFullParams* ) override { return E_NOTIMPL; }
			HRESULT timingsPrint() override { return S_OK; }
			HRESULT timingsReset() override { return S_OK; }
		};

		struct Stream
		{
			uint32_t index = 0;
			const float* pcm = nullptr;
			int64_t nSamples = 0;
			sFullParams params{};
			StreamContext* ctx = nullptr;
			std::vector<int> promptPast;
			TokenTimestamper stamper;
			std::unique_ptr<StreamRun> run;
			void *pcmDev = nullptr, *melDev = nullptr;
			int64_t melLen = 0;
			// the window of the current round
			std::vector<int> prompt;
			std::unique_ptr<WindowScan> scan;
			HRESULT status = S_OK;
			// language "auto": the stream waits in its slot, not begun, until the group's next detection pre-pass has named its language
			bool needsLanguage = false;
			int languageId = -1;
			float languageP = 0;
			// decoding fallback: the plan of the window in the slot, the greedy attempt's no-speech probability, what became of the windows so far.
			// retry: the window failed its last attempt and is decoded again next round -- it keeps prompt and seek and gets a fresh scan
			std::unique_ptr<fallback::FallbackPlan> plan;
			bool retry = false;
			sWindowStats window{};
			std::vector<sWindowStats> stats;
			// speech only: the spans the stream's spectrogram was taken from, relative to the stream's first sample, and the way from its clock back to the
			// stream's (empty: the clocks are the same)
			std::vector<speechRules::Span> spans;
			speechRules::TimeMap map;
		};

		// Device buffers of the streams (PCM, spectrograms), recycled: hipFree waits for the whole device, i.e. for the OTHER group's
		// queued chunk or encoder, so nothing is freed while a run is under way -- a retired stream's buffers serve the next stream.
		class BufferPool
		{
			struct Buf { void* dev; int64_t bytes; };
			std::vector<Buf> idle;
			std::map<void*, int64_t> sizes;
		public:
			HRESULT acquire( int64_t bytes, void*& dev )
			{
				int best = -1;
				for( int i = 0; i < (int)idle.size(); i++ )
					if( idle[ i ].bytes >= bytes && ( best < 0 || idle[ i ].bytes < idle[ best ].bytes ) ) best = i;
				if( best >= 0 && idle[ best ].bytes <= 2 * bytes + 65536 )
				{
					dev = idle[ best ].dev;
					idle.erase( idle.begin() + best );
					return S_OK;
				}
				CHECK_WH( wh_buffer_alloc( bytes, &dev ) );
				sizes[ dev ] = bytes;
				return S_OK;
			}
			void release( void* dev )
			{
				if( dev ) idle.push_back( Buf{ dev, sizes[ dev ] } );
			}
			// only with the device idle (the runner's destructor)
			void freeAll()
			{
				for( auto& kv : sizes ) wh_buffer_free( kv.first );
				sizes.clear();
				idle.clear();
			}
		};
		// What the groups of a runner share: the pool and a one-window context whose stream carries the uploads and spectrograms of
		// newly admitted streams, so that admission waits for its own copies only -- not for a group's queued decode work.
		struct Shared
		{
			wh_context* loader = nullptr;
			BufferPool pool;
		};

		struct Group
		{
			wh_context* gpu = nullptr;
			int slots = 0;
			std::vector<Stream*> slot;
			enum ePhase { Idle, Decoding, Done } phase = Idle;
			int enqueued = 0, fetched = 0, promptMax = 0;
			std::vector<wh_token_data> buf;
			std::vector<int32_t> tokens, lens;
			std::vector<wh_mel_window> windows;
			std::vector<float> langP;
			std::vector<int32_t> langBest;
			// decoding fallback: the rows' sampling parameters of the round, and whether its prompt step gathers the no-speech probabilities
			std::vector<float> temperature, noSpeech;
			std::vector<uint64_t> seed;
			std::vector<uint32_t> nonce;
			bool gathers = false;
			// suppressed tokens: the version of the runner's set this group's context holds (0 = never told: a new context holds none)
			uint32_t suppressVersion = 0;
			// timestamp rules: the version of the runner's switch this group's context holds (0 = never told: a new context has them off)
			uint32_t timestampRulesVersion = 0;
			// boosted phrases: the version of the runner's set this group's context holds (0 = never told: a new context holds none)
			uint32_t boostVersion = 0;
			// no-repeat n-grams: the n this group's context holds (a new context holds 0, off)
			int noRepeatN = 0;
		};

		// One call of iBatchRunner::run over the runner's groups (their wh_contexts outlive the call: KV caches, captured graphs)
		class Scheduler
		{
			const std::shared_ptr<LoadedModel> model;
			iModel* const owner;
			const sFullParams& common;
			const sBatchStream* const descs;
			const uint32_t count;
			iTranscribeResult** const results;
			HRESULT* const perStream;
			std::vector<Group>& groups;
			Shared& shared;
			const int chunk, lookahead;
			const sDecodingFallback* const fallbackParams;	   // nullptr: the feature is off
			const sSpeechFilter* const speechParams;		   // nullptr: the feature is off
			bool loaderBusy = false;
			std::deque<uint32_t> pending;
			HRESULT firstFailure = S_OK;

			void fail( Stream& s, HRESULT hr )
			{
				s.status = hr;
				if( SUCCEEDED( firstFailure ) ) firstFailure = hr;
			}
			// The stream's device buffers go, its transcript becomes results[index]
			void retire( Group& g, int b )
			{
				Stream* s = g.slot[ b ];
				g.slot[ b ] = nullptr;
				shared.pool.release( s->melDev );
				shared.pool.release( s->pcmDev );
				if( perStream ) perStream[ s->index ] = s->status;
				if( SUCCEEDED( s->status ) )
				{
					TranscribeResult* r = new TranscribeResult();
					fillResultData( s->ctx->resultAll, model->vocab, s->ctx->mediaTimeOffset, eResultFlags::Tokens | eResultFlags::Timestamps, *r );
					s->ctx->labelNewSegments();
					r->speakers = s->ctx->speakers;
					r->languageId = s->languageId;
					r->languageP = s->languageP;
					r->windowStats = std::move( s->stats );
					for( const speechRules::Span& sp : s->spans ) r->spans.push_back( sSpeechSpan{ sp.a, sp.b } );
					results[ s->index ] = r;
				}
				s->run.reset();
				s->ctx->Release();
				delete s;
			}
			// Next pending stream -> slot b: PCM to the device, its spectrogram (normalised on the stream's own maximum, like runFull's on
			// its buffer), StreamRun::begin. Returns false when nothing is pending. A stream that ends here (too short, bad parameters)
			// is retired on the spot and the next one is tried.
			bool admit( Group& g, int b )
			{
				while( !pending.empty() )
				{
					const uint32_t i = pending.front();
					pending.pop_front();
					const sBatchStream& d = descs[ i ];
					Stream* s = new Stream();
					s->index = i;
					s->params = d.params ? *d.params : common;
					s->ctx = new StreamContext( owner, model->vocab );
					g.slot[ b ] = s;
					const int64_t total = d.buffer ? (int64_t)d.buffer->countSamples() : 0;
					const float* const mono = d.buffer ? d.buffer->getPcmMono() : nullptr;
					if( !d.buffer || d.firstSample < 0 || d.firstSample > total || d.countSamples < 0 || d.firstSample + d.countSamples > total || ( total > 0 && !mono ) )
					{
						logError( "runFullBatch: stream %u names samples outside its buffer", i );
						fail( *s, E_INVALIDARG );
						retire( g, b );
						continue;
					}
					s->nSamples = d.countSamples ? d.countSamples : total - d.firstSample;
					s->pcm = mono ? mono + d.firstSample : nullptr;
					if( const float* const st = d.buffer->getPcmStereo() )
					{
						s->ctx->stereoPcm = st + 2 * d.firstSample;
						s->ctx->stereoFrames = (size_t)s->nSamples;
					}
					int64_t bufferTime = 0;
					d.buffer->getTime( bufferTime );
					s->ctx->mediaTimeOffset = bufferTime + d.firstSample * 10000000ll / 16000;
					s->melLen = s->nSamples / 160;
					HRESULT hr = S_OK;
					if( speechParams )
					{
						// speech only: the stream is filtered HERE, on the context that uploads it. Its spectrogram is taken from the packed speech -- the loader's own
						// buffer, which the next admission overwrites behind this spectrogram on the same stream -- and a stream without speech never takes a slot.
						hr = admitSpeechOnly( *s );
						if( hr == S_FALSE )
						{
							logInfo( "runFullBatch: the speech filter found no speech in stream %u (%.2f s); nothing to transcribe", i, (double)s->nSamples / 16000.0 );
							retire( g, b );
							continue;
						}
					}
					else if( s->melLen > 0 )
					{
						// enqueued on the loader's stream; startRound waits for it once, after the last admission of the round
						int64_t got = 0;
						wh_context_bind( shared.loader );
						hr = shared.pool.acquire( s->nSamples * 4, s->pcmDev );
						if( SUCCEEDED( hr ) ) hr = shared.pool.acquire( s->melLen * model->hp.n_mels * 4, s->melDev );
						if( SUCCEEDED( hr ) && ( 0 != wh_buffer_upload_async( shared.loader, s->pcmDev, s->pcm, s->nSamples * 4 ) ||
							0 != wh_mel_spectrogram( shared.loader, (const float*)s->pcmDev, s->nSamples, (float*)s->melDev, &got ) ) )
							hr = hrFromStatus( -1, "runFullBatch: stream admission" );
						loaderBusy = true;
					}
					if( SUCCEEDED( hr ) && model->vocab.isMultilingual() && isLanguageAuto( s->params.language ) )
					{
						// every stream gets ITS OWN language. Where StreamRun::begin returns before it reads the language (less than a second of
						// audio, parameters it rejects) nothing is detected and begin answers as it does for a named language
						if( languageDetectionMoot( s->params, s->melLen, model->hp ) )
							s->params.language = makeLanguageKey( "en" );
						else if( !g_batchLanguageDetector )
						{
							logError( "runFullBatch: language \"auto\" needs the language detector, which this build of the scheduler was not given" );
							hr = E_NOTIMPL;
						}
						else
						{
							s->needsLanguage = true;	// begun by detectLanguages(), in the pre-pass of the round that admitted it
							return true;
						}
					}
					if( SUCCEEDED( hr ) ) hr = begin( *s );
					if( hr != S_OK )
					{
						if( FAILED( hr ) ) fail( *s, hr );
						else s->status = hr;	  // S_FALSE: shorter than a second, an empty transcript (ContextImpl.cpp:469-473)
						retire( g, b );
						continue;
					}
					return true;
				}
				return false;
			}

			HRESULT begin( Stream& s )
			{
				if( s.params.flag( eFullParamsFlags::TokenTimestamps ) ) s.stamper.begin( s.pcm, (size_t)s.nSamples );
				const sProgressSink none{ nullptr, nullptr };
				s.run.reset( new StreamRun( s.params, model->vocab, model->hp, s.ctx, none, s.ctx->resultAll, s.promptPast, &s.stamper ) );
				// speech only: the stream's own map; its offset in the buffer is added where the times are reported (the context's mediaTimeOffset)
				if( !s.map.empty() ) s.run->setTimeMap( &s.map );
				return s.run->begin( s.melLen );
			}

			// Admission with the speech filter on: upload, filter, the spectrogram of the packed speech. S_FALSE: no speech, nothing to transcribe.
			HRESULT admitSpeechOnly( Stream& s )
			{
				if( s.params.offset_ms != 0 || s.params.duration_ms != 0 )
				{
					logError( "runFullBatch: offset_ms and duration_ms are not available with the speech filter (setBatchSpeechFilter) on [stream %u]", s.index );
					return E_INVALIDARG;
				}
				if( s.params.flag( eFullParamsFlags::TokenTimestamps ) )
				{
					logError( "runFullBatch: eFullParamsFlags::TokenTimestamps is not available with the speech filter (setBatchSpeechFilter) on [stream %u]", s.index );
					return E_NOTIMPL;
				}
				if( s.melLen <= 0 ) return S_FALSE;
				wh_context_bind( shared.loader );
				CHECK( shared.pool.acquire( s.nSamples * 4, s.pcmDev ) );
				CHECK_WH( wh_buffer_upload_async( shared.loader, s.pcmDev, s.pcm, s.nSamples * 4 ) );
				loaderBusy = true;
				const wh_speech_params p{ speechParams->minSilenceFrames, speechParams->minSpeechFrames, speechParams->padFrames };
				// the spans of a recording are at least a frame long and a frame apart
				const int cap = (int)std::min<int64_t>( 65536, s.nSamples / ( 2 * vad::FRAME_SAMPLES ) + 1 );
				std::vector<int64_t> flat( (size_t)cap * 2 );
				int count = 0;
				const float* packed = nullptr;
				int64_t nPacked = 0;
				CHECK_WH( g_batchSpeechPacker( shared.loader, (const float*)s.pcmDev, s.nSamples, nullptr, &p, &packed, nullptr, &nPacked, flat.data(), cap, &count ) );
				for( int k = 0; k < count; k++ ) s.spans.push_back( speechRules::Span{ flat[ (size_t)k * 2 ], flat[ (size_t)k * 2 + 1 ] } );
				if( count == 0 || !packed ) return S_FALSE;
				if( !speechRules::coversAll( s.spans, s.nSamples ) ) s.map.assign( s.spans );
				s.melLen = nPacked / 160;
				if( s.melLen <= 0 ) return S_OK;	// StreamRun::begin answers S_FALSE: less than a second
				CHECK( shared.pool.acquire( s.melLen * model->hp.n_mels * 4, s.melDev ) );
				int64_t got = 0;
				CHECK_WH( wh_mel_spectrogram( shared.loader, packed, nPacked, (float*)s.melDev, &got ) );
				return S_OK;
			}

			// The detection pre-pass of a round (the "auto" branch of whisper_full, whisper.cpp:2788-2801, for a lock-step batch): the windows at FRAME 0
			// of the streams that wait for their language -- whatever their offset_ms; every other slot a window of zeros -- are ONE encoder batch with the
			// model's full audio context and ONE call of the detector; each stream then begins with its own language key (the prompts of a round are
			// ragged anyway). The group is idle here: nothing of a window in progress is lost. The first windows are encoded again by the round itself
			// (one encoder batch more per admission wave, not per stream; the results do not depend on it).
			HRESULT detectLanguages( Group& g )
			{
				if( loaderBusy )
				{
					CHECK_WH( wh_context_synchronize( shared.loader ) );
					loaderBusy = false;
				}
				const int nDev = languageTokenCount( model->hp ), n = std::min( nDev, (int)languageList().length );
				g.windows.assign( (size_t)g.slots, wh_mel_window{ nullptr, 0, 0, 0 } );
				for( int b = 0; b < g.slots; b++ )
					if( g.slot[ b ] && g.slot[ b ]->needsLanguage ) g.windows[ b ] = wh_mel_window{ (const float*)g.slot[ b ]->melDev, g.slot[ b ]->melLen, 0, 0 };
				g.langP.assign( (size_t)g.slots * nDev, 0.0f );
				g.langBest.assign( (size_t)g.slots, 0 );
				CHECK_WH( wh_context_set_audio_ctx( g.gpu, 0 ) );
				CHECK_WH( wh_encode_windows( g.gpu, g.windows.data(), g.slots ) );
				CHECK_WH( g_batchLanguageDetector( g.gpu, g.slots, g.langP.data(), g.langBest.data() ) );
				CHECK_WH( wh_context_set_audio_ctx( g.gpu, common.audio_ctx ) );
				std::vector<float> lp( (size_t)n );
				for( int b = 0; b < g.slots; b++ )
				{
					Stream* s = g.slot[ b ];
					if( !s || !s->needsLanguage ) continue;
					s->needsLanguage = false;
					s->languageId = finishLanguageProbs( g.langP.data() + (size_t)b * nDev, n, lp.data() );
					if( s->languageId < 0 )
					{
						fail( *s, E_UNEXPECTED );
						retire( g, b );
						continue;
					}
					s->languageP = lp[ (size_t)s->languageId ];
					const std::string code = languageCode( s->languageId );
					s->params.language = makeLanguageKey( code.c_str() );
					logInfo( "whisper_full: auto-detected language: %s (p = %f) [stream %u]", code.c_str(), s->languageP, s->index );
					const HRESULT hr = begin( *s );
					if( hr != S_OK )
					{
						if( FAILED( hr ) ) fail( *s, hr );
						else s->status = hr;
						retire( g, b );
					}
				}
				return S_OK;
			}

			// Every slot's next window; streams that end here leave and their slots are refilled. Returns true when a slot holds a stream that waits for
			// its language: the caller runs the detection pre-pass and calls again (slots the pre-pass emptied are refilled then; a stream that has
			// its window of this round already keeps it).
			bool nextWindows( Group& g, bool& any )
			{
				bool detect = false;
				for( int b = 0; b < g.slots; b++ )
				{
					while( true )
					{
						if( !g.slot[ b ] && !admit( g, b ) ) break;
						Stream& s = *g.slot[ b ];
						if( s.needsLanguage ) { detect = true; break; }
						if( s.scan ) break;
						if( s.retry )
						{
							// this slot has its window: the same prompt at the same seek, scanned afresh
							s.retry = false;
							s.scan.reset( new WindowScan( s.run->fullParams(), model->vocab, s.run->seek, s.run->seekEnd(), s.run->maxTokens() ) );
							any = true;
							break;
						}
						const HRESULT hr = s.run->nextWindow( s.prompt );
						if( hr == S_OK )
						{
							s.scan.reset( new WindowScan( s.run->fullParams(), model->vocab, s.run->seek, s.run->seekEnd(), s.run->maxTokens() ) );
							if( fallbackParams )
							{
								s.plan.reset( new fallback::FallbackPlan( *fallbackParams, s.run->seek ) );
								s.window = sWindowStats{};
								s.window.seek = s.run->seek;
							}
							any = true;
							break;
						}
						if( FAILED( hr ) ) fail( s, hr );
						else
						{
							const HRESULT hrEnd = s.run->end();
							if( FAILED( hrEnd ) ) fail( s, hrEnd );
							// every window dropped as silence: an empty transcript, reported the way a recording too short to transcribe is
							else if( !s.stats.empty() && std::all_of( s.stats.begin(), s.stats.end(), []( const sWindowStats& w ) { return w.skipped != 0; } ) ) s.status = S_FALSE;
						}
						retire( g, b );
					}
				}
				return detect;
			}

			// The round: every slot's next window, then the round's device work is enqueued.
			HRESULT startRound( Group& g )
			{
				bool any = false;
				while( nextWindows( g, any ) ) CHECK( detectLanguages( g ) );
				if( loaderBusy )
				{
					CHECK_WH( wh_context_synchronize( shared.loader ) );
					loaderBusy = false;
				}
				if( !any )
				{
					g.phase = Group::Done;
					return S_OK;
				}
				// one encoder batch: each slot its own spectrogram at its own seek; an idle slot is a window of zeros with a one-token prompt
				const int sot = model->vocab.token_sot;
				g.promptMax = 1;
				for( int b = 0; b < g.slots; b++ )
					if( g.slot[ b ] ) g.promptMax = std::max( g.promptMax, (int)g.slot[ b ]->prompt.size() );
				g.tokens.assign( (size_t)g.slots * g.promptMax, 0 );
				g.lens.assign( (size_t)g.slots, 1 );
				g.windows.assign( (size_t)g.slots, wh_mel_window{ nullptr, 0, 0, 0 } );
				for( int b = 0; b < g.slots; b++ )
				{
					int32_t* const row = g.tokens.data() + (size_t)b * g.promptMax;
					const Stream* s = g.slot[ b ];
					if( !s ) { row[ 0 ] = sot; continue; }
					std::copy( s->prompt.begin(), s->prompt.end(), row );
					g.lens[ b ] = (int32_t)s->prompt.size();
					g.windows[ b ] = wh_mel_window{ (const float*)s->melDev, s->melLen, (int32_t)s->run->seek, 0 };
				}
				CHECK_WH( wh_encode_windows( g.gpu, g.windows.data(), g.slots ) );
				if( fallbackParams )
				{
					// every row at its own attempt: its plan's temperature and nonce, the seed moved by the stream's index (the chunks of one recording all sit at
					// seek 0 and must not share draws); an idle slot is greedy. The no-speech probability is the greedy attempt's: gathered when a slot is at its first.
					// Uploaded behind what the stream holds: a chunk of the last round decoded in vain still reads the old values.
					g.temperature.assign( (size_t)g.slots, 0.0f );
					g.seed.assign( (size_t)g.slots, 0 );
					g.nonce.assign( (size_t)g.slots, 0 );
					g.gathers = false;
					for( int b = 0; b < g.slots; b++ )
					{
						const Stream* s = g.slot[ b ];
						if( !s ) continue;
						g.temperature[ b ] = s->plan->temperature();
						g.seed[ b ] = s->plan->seed() + s->index;
						g.nonce[ b ] = s->plan->nonce();
						g.gathers = g.gathers || s->plan->attemptIndex() == 0;
					}
					CHECK_WH( g_batchSamplingHooks->setRowSampling( g.gpu, g.slots, g.temperature.data(), g.seed.data(), g.nonce.data() ) );
					CHECK_WH( g_batchSamplingHooks->setNoSpeech( g.gpu, g.gathers ? 1 : 0 ) );
				}
				const int room = model->hp.n_text_ctx - g.promptMax;
				const int n0 = std::max( 0, std::min( chunk, room ) );
				CHECK_WH( wh_decode_window_start_ragged( g.gpu, g.slots, g.tokens.data(), g.lens.data(), g.promptMax, n0, 1, 1 ) );
				g.enqueued = 1 + n0;
				g.fetched = 0;
				// lookahead: chunks kept queued BEHIND the one the host waits for. 0 = a chunk is enqueued only once the previous one has
				// been scanned: the stream idles for the host's reaction (a poll + a few graph launches, under the other group's work)
				// and at most one chunk is decoded past the end of a round; 1 = the device never waits, up to two chunks are
				for( int k = 0; k < lookahead; k++ ) CHECK( enqueue( g ) );
				g.phase = Group::Decoding;
				return S_OK;
			}
			HRESULT enqueue( Group& g )
			{
				const int room = model->hp.n_text_ctx - ( g.promptMax + g.enqueued - 1 );
				const int n = std::min( chunk, room );
				if( n <= 0 ) return S_FALSE;
				CHECK_WH( wh_decode_window_continue( g.gpu, n ) );
				g.enqueued += n;
				return S_OK;
			}
			// samples the next fetch of this group takes: the first sample alone, then chunk by chunk
			int nextCount( const Group& g ) const { return g.fetched == 0 ? std::min( g.enqueued, 1 + chunk ) : std::min( chunk, g.enqueued - g.fetched ); }

			HRESULT consume( Group& g )
			{
				const int n = nextCount( g );
				if( n <= 0 )
				{
					// n_text_ctx reached with windows still open: WindowScan's own bound (n_text_ctx / 2 - 4 tokens) fires first for every
					// prompt the host loop can build, so this is unreachable; close the round rather than spin
					return finishRound( g );
				}
				g.buf.resize( (size_t)n * g.slots );
				CHECK_WH( wh_decode_window_fetch( g.gpu, g.fetched, n, g.buf.data() ) );
				g.fetched += n;
				bool open = false;
				for( int b = 0; b < g.slots; b++ )
				{
					Stream* s = g.slot[ b ];
					if( !s || s->scan->over ) continue;
					for( int k = 0; k < n && !s->scan->over; k++ )
					{
						const wh_token_data& t = g.buf[ (size_t)k * g.slots + b ];
						TokenData td;
						td.id = t.id; td.tid = t.tid; td.p = t.p; td.pt = t.pt; td.ptsum = t.ptsum;
						s->scan->feed( td );
					}
					open = open || !s->scan->over;
				}
				if( !open ) return finishRound( g );
				while( g.enqueued - g.fetched < ( 1 + lookahead ) * chunk )
					if( enqueue( g ) != S_OK ) break;
				return S_OK;
			}
			HRESULT finishRound( Group& g )
			{
				if( fallbackParams && g.gathers )
				{
					g.noSpeech.assign( (size_t)g.slots, 0.0f );
					CHECK_WH( g_batchSamplingHooks->readNoSpeech( g.gpu, g.noSpeech.data() ) );
				}
				for( int b = 0; b < g.slots; b++ )
				{
					Stream* s = g.slot[ b ];
					if( !s ) continue;
					if( !s->scan->over ) s->scan->failed = s->scan->over = true;	// see consume(): not reachable through the host loop's prompts
					if( fallbackParams )
					{
						// scored exactly as iContext::runFull scores an attempt; the plan says what becomes of the window
						WindowScan& scan = *s->scan;
						sWindowStats& ws = s->window;
						if( s->plan->attemptIndex() == 0 ) ws.noSpeech = g.noSpeech[ b ];
						fallback::Attempt a;
						a.scanFailed = scan.failed;
						a.resultLen = std::min( scan.resultLen, (int)scan.tokens.size() );
						a.scores = fallback::score( scan.tokens.data(), a.resultLen );
						a.noSpeech = ws.noSpeech;
						ws.attempts = s->plan->attempts();
						ws.temperature = s->plan->temperature();
						ws.avgLogprob = a.scores.avgLogprob;
						ws.entropy = a.scores.entropy;
						const fallback::eVerdict verdict = s->plan->judge( a );
						if( verdict == fallback::eVerdict::Retry )
						{
							// the window stays in its slot: the next round decodes it again at the plan's next temperature
							s->scan.reset();
							s->retry = true;
							continue;
						}
						if( verdict == fallback::eVerdict::Skip )
						{
							// silence: no segments, nothing for the next window's prompt, the stream moves on by the scan's seekDelta
							scan.tokens.clear();
							scan.resultLen = 0;
							ws.skipped = 1;
						}
						s->stats.push_back( ws );
					}
					const HRESULT hr = s->run->finishWindow( *s->scan );
					s->ctx->labelNewSegments();
					s->scan.reset();
					if( FAILED( hr ) )
					{
						fail( *s, hr );
						retire( g, b );
					}
				}
				g.phase = Group::Idle;
				return S_OK;
			}

		public:
			Scheduler( const std::shared_ptr<LoadedModel>& m, iModel* o, const sFullParams& p, const sBatchStream* d, uint32_t n, iTranscribeResult** r, HRESULT* per,
				std::vector<Group>& grp, Shared& sh, int chunk_, int lookahead_, const sDecodingFallback* fallback_, const sSpeechFilter* speech_ )
				: model( m ), owner( o ), common( p ), descs( d ), count( n ), results( r ), perStream( per ), groups( grp ), shared( sh ), chunk( chunk_ ), lookahead( lookahead_ ),
				fallbackParams( fallback_ ), speechParams( speech_ ) {}
			~Scheduler()
			{
				// a failure left streams in their slots: their buffers go, the device work they queued is awaited
				for( Group& g : groups )
				{
					for( int b = 0; b < (int)g.slot.size(); b++ )
						if( g.slot[ b ] )
						{
							g.slot[ b ]->status = E_FAIL;
							retire( g, b );
						}
					if( g.gpu ) wh_context_synchronize( g.gpu );
					g.phase = Group::Idle;
				}
				if( shared.loader ) wh_context_synchronize( shared.loader );
			}
			HRESULT run( int slots, int nGroups )
			{
				for( uint32_t i = 0; i < count; i++ )
				{
					results[ i ] = nullptr;
					if( perStream ) perStream[ i ] = S_OK;
					pending.push_back( i );
				}
				for( int gi = 0; gi < (int)groups.size(); gi++ )
				{
					Group& g = groups[ gi ];
					g.slots = slots;
					g.slot.assign( (size_t)slots, nullptr );
					g.phase = gi < nGroups ? Group::Idle : Group::Done;
				}
				while( true )
				{
					bool progressed = false, alive = false;
					for( Group& g : groups )
					{
						if( g.phase == Group::Idle )
						{
							CHECK( startRound( g ) );
							progressed = true;
						}
						else if( g.phase == Group::Decoding )
						{
							const int n = nextCount( g );
							const int ready = n > 0 ? wh_decode_window_ready( g.gpu, g.fetched, n ) : 1;
							if( ready < 0 ) return hrFromStatus( ready, "wh_decode_window_ready" );
							if( ready )
							{
								CHECK( consume( g ) );
								progressed = true;
							}
						}
						alive = alive || g.phase != Group::Done;
					}
					if( !alive ) break;
					if( !progressed ) std::this_thread::sleep_for( std::chrono::microseconds( 50 ) );
				}
				return firstFailure;
			}
		};

		// iBatchRunner: the groups' device contexts (KV caches for maxSlots windows each, captured decode graphs) live as long as the
		// runner, so a service that transcribes batch after batch pays for them once.
		class BatchRunner : public ComObject<iBatchRunner>
		{
			const std::shared_ptr<LoadedModel> model;
			iModel* const owner;
			uint32_t maxSlots = 64, nGroups = 2;
			int chunk = 4, lookahead = 0;
			std::vector<Group> groups;
			Shared shared;
			// Whisper::setBatchDecodingFallback: off unless set. modesDirty: a run with the feature on left the groups' contexts in its modes
			bool fallbackOn = false, modesDirty = false;
			sDecodingFallback fallbackParams;
			// Whisper::setBatchSuppressedTokens: one set for every stream; each group's context is told once, before the first round that follows a change
			std::vector<int32_t> suppressIds;
			uint32_t suppressVersion = 0;
			// Whisper::setBatchTimestampRules: one switch for every stream; each group's context is told once, before the first round that follows a change
			bool timestampRulesOn = false;
			uint32_t timestampRulesVersion = 0;
			// Whisper::setBatchBoostedPhrases: one set for every stream; each group's context is told once, before the first round that follows a change
			phraseBoost::Set boostSet;
			uint32_t boostVersion = 0;
			// Whisper::setBatchNoRepeatNgram: one n for every stream, 0 = off; a group's context is told before the first round in which it holds another n
			int noRepeatN = 0;
			// Whisper::setBatchSpeechFilter: off unless set; every stream of a run is filtered when it is admitted
			bool speechOn = false;
			sSpeechFilter speechParams{};
		public:
			// The setters answer in one order: the argument check (optionRules.h), E_NOTIMPL without the device entry, "nothing changes", then the new version
			HRESULT setBoosted( const sBoostedPhrases* p )
			{
				phraseBoost::Set set;
				CHECK( optionRules::checkBoosted( "setBatchBoostedPhrases", p, model->vocab.token_eot, set ) );
				if( set.count() && !g_batchBoost ) return optionRules::notGiven( "setBatchBoostedPhrases", "phrase filter" );
				if( set.count() == 0 && boostSet.count() == 0 ) return S_OK;
				boostSet = std::move( set );
				boostVersion++;
				return S_OK;
			}
			HRESULT setSpeech( const sSpeechFilter* p )
			{
				if( !p ) { speechOn = false; return S_OK; }
				CHECK( optionRules::checkSpeechFilter( "setBatchSpeechFilter", *p ) );
				if( !g_batchSpeechPacker ) return optionRules::notGiven( "setBatchSpeechFilter", "speech packer" );
				speechParams = *p;
				speechOn = true;
				return S_OK;
			}
			HRESULT setNoRepeat( int n )
			{
				CHECK( optionRules::checkNoRepeat( "setBatchNoRepeatNgram", n ) );
				if( n && !g_batchNoRepeat ) return optionRules::notGiven( "setBatchNoRepeatNgram", "n-gram filter" );
				noRepeatN = n;
				return S_OK;
			}
			HRESULT setTimestampRulesMode( bool on )
			{
				if( on && !g_batchTimestampRules ) return optionRules::notGiven( "setBatchTimestampRules", "timestamp filter" );
				if( on == timestampRulesOn ) return S_OK;
				timestampRulesOn = on;
				timestampRulesVersion++;
				return S_OK;
			}
			HRESULT setSuppressed( const int32_t* ids, uint32_t count )
			{
				CHECK( optionRules::checkSuppressed( "setBatchSuppressedTokens", ids, count, model->vocab.token_eot ) );
				if( count && !g_batchSuppress ) return optionRules::notGiven( "setBatchSuppressedTokens", "logit filter" );
				if( count == 0 && suppressIds.empty() ) return S_OK;
				suppressIds.assign( ids, ids + count );
				suppressVersion++;
				return S_OK;
			}
			HRESULT setFallback( const sDecodingFallback* p )
			{
				if( !p ) { fallbackOn = false; return S_OK; }
				CHECK( optionRules::checkFallback( "setBatchDecodingFallback", *p ) );
				if( !g_batchSamplingHooks ) return optionRules::notGiven( "setBatchDecodingFallback", "per-row sampler" );
				fallbackParams = *p;
				fallbackOn = true;
				return S_OK;
			}
			BatchRunner( const std::shared_ptr<LoadedModel>& m, iModel* o, const sBatchSetup* setup ) : model( m ), owner( o )
			{
				owner->AddRef();
				if( setup && setup->maxSlots ) maxSlots = setup->maxSlots;
				if( setup && setup->groups ) nGroups = setup->groups;
				if( setup && setup->greedyChunk ) chunk = (int)setup->greedyChunk;
				if( setup && ( setup->flags & 1u ) ) lookahead = 1;
				if( const char* e = getenv( "WHISPER_BATCH_SLOTS" ) ) maxSlots = (uint32_t)std::max( 1, atoi( e ) );
				if( const char* e = getenv( "WHISPER_BATCH_GROUPS" ) ) nGroups = (uint32_t)std::max( 1, atoi( e ) );
				if( const char* e = getenv( "WHISPER_BATCH_CHUNK" ) ) chunk = atoi( e );
				if( const char* e = getenv( "WHISPER_BATCH_LOOKAHEAD" ) ) lookahead = atoi( e ) ? 1 : 0;
				chunk = std::max( 1, std::min( chunk, 64 ) );
				maxSlots = std::max<uint32_t>( 1, std::min<uint32_t>( maxSlots, 512 ) );
				nGroups = std::max<uint32_t>( 1, std::min<uint32_t>( nGroups, 8 ) );
			}
			~BatchRunner() override
			{
				for( Group& g : groups )
					if( g.gpu ) wh_context_synchronize( g.gpu );
				if( shared.loader )
				{
					wh_context_synchronize( shared.loader );
					shared.pool.freeAll();
					wh_context_destroy( shared.loader );
				}
				for( Group& g : groups )
					if( g.gpu ) wh_context_destroy( g.gpu );
				owner->Release();
			}
			// Whisper::scoreBatch: the requests that pass their checks (scoreRequest.h), up to maxSlots per pass in request order, on the first group's context.
			// One pass = the clips' spectrograms on the loader's stream, one encoder batch at seek 0 with the full audio context, one call of the scorer.
			HRESULT score( const sScoreRequest* requests, uint32_t count, sTokenScore* const* scores, HRESULT* perRequest )
			{
				if( count && ( !requests || !scores ) ) return E_POINTER;
				if( !g_batchScorer ) return optionRules::notGiven( "scoreBatch", "scorer" );
				const score::Limits lim{ model->hp.n_vocab, model->vocab.token_eot, model->vocab.token_not, model->hp.n_text_ctx };
				std::vector<HRESULT> status( count, S_OK );
				std::vector<score::Row> rows( count );
				std::vector<int64_t> samples( count, 0 );
				for( uint32_t i = 0; i < count; i++ )
				{
					const sScoreRequest& r = requests[ i ];
					HRESULT& hr = status[ i ];
					if( !r.buffer || !r.buffer->getPcmMono() || !scores[ i ] ) hr = E_POINTER;
					if( SUCCEEDED( hr ) ) hr = score::clipRange( r.buffer->countSamples(), r.firstSample, r.countSamples, samples[ i ] );
					if( SUCCEEDED( hr ) ) hr = score::buildRow( lim, r.prompt, r.promptCount, r.tokens, r.count, r.flags, rows[ i ] );
					if( SUCCEEDED( hr ) && rows[ i ].align )
					{
						logError( "scoreBatch: forced alignment (flag 1) is not available in a batch runner; use scoreTokens" );
						hr = E_NOTIMPL;
					}
				}
				HRESULT first = S_OK;
				auto fail = [ & ]( uint32_t i, HRESULT hr ) { status[ i ] = hr; };
				const std::vector<std::vector<uint32_t>> passes = score::packPasses( status, maxSlots );
				if( !passes.empty() )
				{
					if( groups.empty() )
					{
						Group g;
						CHECK_WH( wh_context_create( model->gpu, (int)maxSlots, nullptr, &g.gpu ) );
						groups.push_back( std::move( g ) );
					}
					if( !shared.loader ) CHECK_WH( wh_context_create( model->gpu, 1, nullptr, &shared.loader ) );
					CHECK_WH( wh_context_set_audio_ctx( groups[ 0 ].gpu, 0 ) );
				}
				for( const std::vector<uint32_t>& pass : passes )
				{
					wh_context* const gpu = groups[ 0 ].gpu;
					std::vector<void*> held;
					std::vector<wh_mel_window> windows( pass.size() );
					HRESULT hr = S_OK;
					for( size_t s = 0; s < pass.size() && SUCCEEDED( hr ); s++ )
					{
						const sScoreRequest& r = requests[ pass[ s ] ];
						const int64_t n = samples[ pass[ s ] ], melLen = n / 160;
						void *pcmDev = nullptr, *melDev = nullptr;
						hr = shared.pool.acquire( n * 4, pcmDev );
						if( SUCCEEDED( hr ) ) held.push_back( pcmDev );
						if( SUCCEEDED( hr ) ) hr = shared.pool.acquire( melLen * model->hp.n_mels * 4, melDev );
						if( SUCCEEDED( hr ) ) held.push_back( melDev );
						int64_t got = 0;
						if( SUCCEEDED( hr ) && ( 0 != wh_buffer_upload_async( shared.loader, pcmDev, r.buffer->getPcmMono() + r.firstSample, n * 4 ) ||
							0 != wh_mel_spectrogram( shared.loader, (const float*)pcmDev, n, (float*)melDev, &got ) ) )
							hr = hrFromStatus( -1, "scoreBatch: spectrogram" );
						windows[ s ] = wh_mel_window{ (const float*)melDev, melLen, 0, 0 };
					}
					const score::PassArgs a = score::packTokens( pass, rows );
					std::vector<wh_token_score> recs( pass.size() * (size_t)a.nMax );
					if( SUCCEEDED( hr ) && 0 != wh_context_synchronize( shared.loader ) ) hr = hrFromStatus( -1, "scoreBatch: wh_context_synchronize" );
					if( SUCCEEDED( hr ) ) { const int rc = wh_encode_windows( gpu, windows.data(), (int)pass.size() ); if( rc ) hr = hrFromStatus( rc, "scoreBatch: wh_encode_windows" ); }
					if( SUCCEEDED( hr ) ) { const int rc = g_batchScorer( gpu, (int)pass.size(), a.tokens.data(), a.lens.data(), a.first.data(), a.nMax, recs.data() ); if( rc ) hr = hrFromStatus( rc, "scoreBatch: the scorer" ); }
					wh_context_synchronize( gpu );	  // the encoder has read the spectrograms before their buffers go back to the pool
					for( void* p : held ) shared.pool.release( p );
					if( SUCCEEDED( hr ) ) score::unpackRecords( pass, rows, a, recs.data(), scores );
					else
						for( uint32_t r : pass ) fail( r, hr );
				}
				for( uint32_t i = 0; i < count; i++ )
				{
					if( perRequest ) perRequest[ i ] = status[ i ];
					if( FAILED( status[ i ] ) && SUCCEEDED( first ) ) first = status[ i ];
				}
				return first;
			}
			HRESULT run( const sFullParams& params, const sBatchStream* streams, uint32_t count, iTranscribeResult** results, HRESULT* perStream ) override
			{
				if( !results || ( count && !streams ) ) return E_POINTER;
				if( count == 0 ) return S_OK;
				// the lock-step batch decodes greedily (one sequence per stream); beam search is iContext::runFull's (hypotheses of ONE window in lock step)
				bool beam = params.strategy == eSamplingStrategy::BeamSearch;
				for( uint32_t i = 0; i < count; i++ ) beam = beam || ( streams[ i ].params && streams[ i ].params->strategy == eSamplingStrategy::BeamSearch );
				if( beam )
				{
					logError( "runFullBatch: eSamplingStrategy::BeamSearch is not available in a lock-step batch; use iContext::runFull" );
					return E_NOTIMPL;
				}
				// AlignTokens: the scheduler keeps two batches in flight and a group's caches may be gone when a window is scanned (a follow-up)
				bool align = params.flag( eFullParamsFlags::AlignTokens );
				for( uint32_t i = 0; i < count; i++ ) align = align || ( streams[ i ].params && streams[ i ].params->flag( eFullParamsFlags::AlignTokens ) );
				if( align )
				{
					logError( "runFullBatch: eFullParamsFlags::AlignTokens is not available in a lock-step batch; use iContext::runFull" );
					return E_NOTIMPL;
				}
				// streams dealt evenly: no more groups than hold two streams each, every group the same number of slots
				const uint32_t useGroups = std::max<uint32_t>( 1, std::min<uint32_t>( nGroups, count / 2 ) );
				const uint32_t slots = std::max<uint32_t>( 1, std::min<uint32_t>( maxSlots, ( count + useGroups - 1 ) / useGroups ) );
				while( groups.size() < useGroups )
				{
					Group g;
					CHECK_WH( wh_context_create( model->gpu, (int)maxSlots, nullptr, &g.gpu ) );
					groups.push_back( std::move( g ) );
				}
				if( !shared.loader ) CHECK_WH( wh_context_create( model->gpu, 1, nullptr, &shared.loader ) );
				// one sFullParams for every stream of the batch: its audio_ctx is the groups' (ContextImpl.cpp:488-489)
				if( params.audio_ctx < 0 || params.audio_ctx > model->hp.n_audio_ctx ) return E_INVALIDARG;
				for( Group& g : groups ) CHECK_WH( wh_context_set_audio_ctx( g.gpu, params.audio_ctx ) );
				// a context is told what changed since it was last told: the set, the rules, the phrases, the n-gram size
				for( Group& g : groups )
				{
					if( g.suppressVersion != suppressVersion && g_batchSuppress )
					{
						CHECK_WH( g_batchSuppress( g.gpu, suppressIds.data(), (int)suppressIds.size() ) );
						g.suppressVersion = suppressVersion;
					}
					if( g.timestampRulesVersion != timestampRulesVersion && g_batchTimestampRules )
					{
						CHECK_WH( g_batchTimestampRules( g.gpu, timestampRulesOn ? 1 : 0 ) );
						g.timestampRulesVersion = timestampRulesVersion;
					}
					if( g.boostVersion != boostVersion && g_batchBoost )
					{
						CHECK_WH( g_batchBoost( g.gpu, boostSet.tokens.data(), boostSet.lens.data(), boostSet.count(), boostSet.nMax, boostSet.boost ) );
						g.boostVersion = boostVersion;
					}
					if( g.noRepeatN != noRepeatN && g_batchNoRepeat )
					{
						CHECK_WH( g_batchNoRepeat( g.gpu, noRepeatN ) );
						g.noRepeatN = noRepeatN;
					}
				}
				if( modesDirty && !fallbackOn )
				{
					// the feature was turned off: the contexts go back to the greedy sampler and gather nothing
					for( Group& g : groups )
					{
						CHECK_WH( g_batchSamplingHooks->setRowSampling( g.gpu, 0, nullptr, nullptr, nullptr ) );
						CHECK_WH( g_batchSamplingHooks->setNoSpeech( g.gpu, 0 ) );
					}
					modesDirty = false;
				}
				modesDirty = modesDirty || fallbackOn;
				Scheduler s( model, owner, params, streams, count, results, perStream, groups, shared, chunk, lookahead, fallbackOn ? &fallbackParams : nullptr,
					speechOn ? &speechParams : nullptr );
				const HRESULT hr = s.run( (int)slots, (int)useGroups );
				if( FAILED( hr ) ) logError( "runFullBatch: failed, HRESULT 0x%08x", (unsigned)hr );
				return hr;
			}
		};
	}	// namespace

	// the options of a runner: the public function on the BatchRunner behind `runner` (optionRules::forward)
	static const char* const NOT_A_RUNNER = "not a runner of this library's createBatchRunner";
	HRESULT runnerScore( iBatchRunner* runner, const sScoreRequest* requests, uint32_t count, sTokenScore* const* scores, HRESULT* perRequest )
	{
		return optionRules::forward<BatchRunner>( runner, "scoreBatch", NOT_A_RUNNER, nullptr,
			[ = ]( BatchRunner& r ) { return r.score( requests, count, scores, perRequest ); } );
	}
	HRESULT createBatchRunner( iModel* model, const sBatchSetup* setup, iBatchRunner** pp )
	{
		if( !model || !pp ) return E_POINTER;
		iModelInternals* mi = nullptr;
		if( FAILED( model->QueryInterface( iModelInternals::iid(), (void**)&mi ) ) || !mi )
		{
			logError( "createBatchRunner: this iModel was not created by this library" );
			return E_INVALIDARG;
		}
		const std::shared_ptr<LoadedModel> lm = mi->loaded();
		mi->Release();
		*pp = new BatchRunner( lm, model, setup );
		return S_OK;
	}

	HRESULT setBatchDecodingFallback( iBatchRunner* runner, const sDecodingFallback* params )
	{
		return optionRules::forward<BatchRunner>( runner, "setBatchDecodingFallback", NOT_A_RUNNER, nullptr,
			[ = ]( BatchRunner& r ) { return r.setFallback( params ); } );
	}
	HRESULT setBatchSuppressedTokens( iBatchRunner* runner, const int32_t* ids, uint32_t count )
	{
		return optionRules::forward<BatchRunner>( runner, "setBatchSuppressedTokens", NOT_A_RUNNER, nullptr,
			[ = ]( BatchRunner& r ) { return r.setSuppressed( ids, count ); } );
	}
	HRESULT setBatchTimestampRules( iBatchRunner* runner, bool on )
	{
		return optionRules::forward<BatchRunner>( runner, "setBatchTimestampRules", NOT_A_RUNNER, nullptr,
			[ = ]( BatchRunner& r ) { return r.setTimestampRulesMode( on ); } );
	}
	HRESULT setBatchBoostedPhrases( iBatchRunner* runner, const sBoostedPhrases* phrases )
	{
		return optionRules::forward<BatchRunner>( runner, "setBatchBoostedPhrases", NOT_A_RUNNER, nullptr,
			[ = ]( BatchRunner& r ) { return r.setBoosted( phrases ); } );
	}
	HRESULT setBatchNoRepeatNgram( iBatchRunner* runner, int n )
	{
		return optionRules::forward<BatchRunner>( runner, "setBatchNoRepeatNgram", NOT_A_RUNNER, nullptr,
			[ = ]( BatchRunner& r ) { return r.setNoRepeat( n ); } );
	}
	HRESULT setBatchSpeechFilter( iBatchRunner* runner, const sSpeechFilter* params )
	{
		return optionRules::forward<BatchRunner>( runner, "setBatchSpeechFilter", NOT_A_RUNNER, nullptr,
			[ = ]( BatchRunner& r ) { return r.setSpeech( params ); } );
	}
	HRESULT getResultSpeechSpans( const iTranscribeResult* result, sSpeechSpan* spans, uint32_t* count )
	{
		if( !result || !count ) return E_POINTER;
		const TranscribeResult* const r = dynamic_cast<const TranscribeResult*>( result );
		if( !r ) return E_INVALIDARG;
		const uint32_t cap = *count;
		*count = (uint32_t)r->spans.size();
		if( !spans ) return S_OK;
		if( cap < r->spans.size() ) return E_BOUNDS;
		std::copy( r->spans.begin(), r->spans.end(), spans );
		return S_OK;
	}
	HRESULT getResultWindowStats( const iTranscribeResult* result, sWindowStats* stats, uint32_t* count )
	{
		if( !result || !count ) return E_POINTER;
		const TranscribeResult* const r = dynamic_cast<const TranscribeResult*>( result );
		if( !r ) return E_INVALIDARG;
		const uint32_t cap = *count;
		*count = (uint32_t)r->windowStats.size();
		if( !stats ) return S_OK;
		if( cap < r->windowStats.size() ) return E_BOUNDS;
		std::copy( r->windowStats.begin(), r->windowStats.end(), stats );
		return S_OK;
	}

	HRESULT runFullBatch( iModel* model, const sFullParams& params, const sBatchStream* streams, uint32_t count, const sBatchSetup* setup,
		iTranscribeResult** results, HRESULT* perStream )
	{
		if( !model || !results || ( count && !streams ) ) return E_POINTER;
		if( count == 0 ) return S_OK;
		iBatchRunner* runner = nullptr;
		sBatchSetup st = setup ? *setup : sBatchSetup{ 0, 0, 0, 0 };
		if( st.maxSlots == 0 ) st.maxSlots = std::min<uint32_t>( 64, count );	 // a one-off call sizes its contexts for what it was given
		CHECK( createBatchRunner( model, &st, &runner ) );
		const HRESULT hr = runner->run( params, streams, count, results, perStream );
		runner->Release();
		return hr;
	}
}
