// iModel / iContext / iTranscribeResult / iAudioBuffer / iMediaFoundation implementations and the functions of whisperApi.h over them (loadModel,
// initMediaFoundation, the decoding options of a context). The flat C mirror of it all is flatApi.cpp's.
//
// Host logic only (plain C++): windows, prompts, stop rules and segment assembly follow the reference's
// ContextImpl::runFullImpl (Whisper/Whisper/ContextImpl.cpp:452-793, itself a port of whisper_full), the arithmetic is
// behind include/whisper_hip.h. Structure here is ours: one WindowDecoder per 30 s window feeds a token stream (filled
// from the device-side greedy loop in chunks) through the reference's stop rules, then SegmentBuilder cuts it at the
// timestamp tokens.
#include <cstdlib>
#include "hostCommon.h"
#include "hostLoop.h"
#include "decodeFallback.h"
#include "batchSampling.h"
#include "batchSuppress.h"
#include "batchTimestampRules.h"
#include "batchBoost.h"
#include "batchNoRepeat.h"
#include "batchSpeech.h"
#include "optionRules.h"
#include "languageDetect.h"
#include "captureRate.h"
#include "scoreRequest.h"
#include "results.h"
#include "wavFormat.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

namespace Whisper
{
	eHostLoopRules g_hostLoopRules = eHostLoopRules::ReferenceCpu;

	namespace
	{
		// greedy steps enqueued per chunk; one chunk always runs behind the one being scanned, so up to two chunks are decoded in
		// vain when a window ends: one sequential 199 s clip through runFull, medium shape, ran at 265 / 308 / 330 / 351 audio-s/s
		// with chunks of 8 / 4 / 2 / 1 in round 3 (1.13 ms per step; a fetch polls the sampler's pinned mailbox, it enqueues
		// nothing). WHISPER_GREEDY_CHUNK overrides (1 .. 64).
		// eSamplingStrategy::BeamSearch: candidates ranked on the host after every step (round 4's decoder, the checker) instead of on the device
		bool g_beamRankingOnHost = []() { const char* e = getenv( "WHISPER_BEAM_HOST" ); return e && atoi( e ) != 0; }();
		static const int GREEDY_CHUNK = []() {
			const char* e = getenv( "WHISPER_GREEDY_CHUNK" );
			const int v = e ? atoi( e ) : 0;
			return v >= 1 && v <= 64 ? v : 1;
		}();


		// ---- iAudioBuffer -----------------------------------------------------------------------------------------
		class AudioBuffer : public ComObject<iAudioBuffer>
		{
		public:
			std::vector<float> mono, stereo;
			uint32_t countSamples() const override { return (uint32_t)mono.size(); }
			const float* getPcmMono() const override { return mono.empty() ? nullptr : mono.data(); }
			const float* getPcmStereo() const override { return stereo.empty() ? nullptr : stereo.data(); }
			HRESULT getTime( int64_t& rdi ) const override { rdi = 0; return S_OK; }
		};

		// ---- iAudioReader -----------------------------------------------------------------------------------------
		// The reference's readers wrap an IMFSourceReader that iContext::runStreamed pulls 10 ms chunks from
		// (Whisper/MF/PcmReader.cpp:393-430). Media Foundation does not exist here; the reader holds the decoded 16 kHz PCM
		// of a WAV file and hands it to runStreamed through a private interface (getReader keeps its slot: E_NOTIMPL).
		// {5d6b0c1e-7f0a-4f53-9f6e-3c1d2a7b9e41}
		struct iPcmSource : public ComLight::IUnknown
		{
			static constexpr ComLight::GUID iid() { return { 0x5d6b0c1e, 0x7f0a, 0x4f53, { 0x9f, 0x6e, 0x3c, 0x1d, 0x2a, 0x7b, 0x9e, 0x41 } }; }
			virtual const std::vector<float>& pcmMono() const = 0;
			// interleaved, 2 floats per frame of pcmMono; empty unless the reader was opened with stereo = true on a source of two channels or more
			virtual const std::vector<float>& pcmStereo() const = 0;
		};
		class WavReader : public iAudioReader, public iPcmSource
		{
			std::atomic<uint32_t> rc{ 1 };
			std::vector<float> mono, stereoPcm;
			bool stereo;
		public:
			WavReader( std::vector<float>&& m, std::vector<float>&& st, bool wantStereo ) : mono( std::move( m ) ), stereoPcm( std::move( st ) ), stereo( wantStereo ) {}
			virtual ~WavReader() = default;
			HRESULT QueryInterface( const ComLight::GUID& riid, void** ppv ) override
			{
				if( !ppv ) return E_POINTER;
				if( riid == iAudioReader::iid() || riid == ComLight::IID_IUnknown ) { *ppv = static_cast<iAudioReader*>( this ); AddRef(); return S_OK; }
				if( riid == iPcmSource::iid() ) { *ppv = static_cast<iPcmSource*>( this ); AddRef(); return S_OK; }
				*ppv = nullptr;
				return E_NOINTERFACE;
			}
			uint32_t AddRef() override { return ++rc; }
			uint32_t Release() override
			{
				const uint32_t r = --rc;
				if( r == 0 ) delete this;
				return r;
			}
			// 100 ns ticks, like MF_PD_DURATION (PcmReader.cpp getDuration)
			HRESULT getDuration( int64_t& rdi ) const override { rdi = (int64_t)mono.size() * 10000000ll / 16000; return S_OK; }
			HRESULT getReader( IMFSourceReader** pp ) const override { if( pp ) *pp = nullptr; return E_NOTIMPL; }
			HRESULT requestedStereo() const override { return stereo ? S_OK : S_FALSE; }
			const std::vector<float>& pcmMono() const override { return mono; }
			const std::vector<float>& pcmStereo() const override { return stereoPcm; }
		};

		// ---- iContext ---------------------------------------------------------------------------------------------
		class ContextImpl : public ComObject<iContext>
		{
			std::shared_ptr<LoadedModel> model;
			iModel* owner;	  // strong reference, like ContextImpl::modelPtr (ContextImpl.h:16)
			wh_context* gpu = nullptr;
			wh_context* gpuBeam = nullptr;	   // eSamplingStrategy::BeamSearch: one window x `beamSlots` hypotheses sharing its cross-attention K/V
			int beamSlots = 0;
			void* melDev = nullptr;
			int64_t melCapacity = 0;
			void* pcmDev = nullptr;
			int64_t pcmCapacity = 0;
			std::vector<Segment> resultAll;
			std::vector<int> promptPast;
			int64_t mediaTimeOffset = 0;
			// detectSpeaker (diarize.h). The reference answers while a run's spectrogram is current (ContextImpl::currentSpectrogram, set and cleared by
			// CurrentSpectrogramRaii around runFullImpl, ContextImpl.cpp:437-465); what it reads from the spectrogram is the stereo PCM, so here the
			// run's stereo PCM is current instead: the caller's buffer (runFull) or the reader's (runStreamed), nullptr when it has none.
			bool runCurrent = false;
			const float* stereoPcm = nullptr;
			size_t stereoFrames = 0;
			mutable std::vector<uint8_t> speakers;	   // per segment of resultAll, see appendSpeakers
			mutable TranscribeResultStatic results;
			// timings, the blocks of ProfileCollection (Whisper/Utils/ProfileCollection.h)
			double msSpectrogram = 0, msEncode = 0, msDecode = 0, msRun = 0;
			int nEncode = 0, nDecodeSteps = 0, nRuns = 0, nSpectrogram = 0, nDecodeWindows = 0;
			TokenTimestamper stamper;	  // TokenTimestamps flag: token-level times + max_len wrapping (host-only post-processing)
			bool gpuProfile = false;	  // WHISPER_PROFILE=1: per-kernel hipEvent timing, printed as the "Compute Shaders" table
			// Whisper::setDecodingFallback (decodeFallback.h): off unless set; what it did with the windows of the last run
			bool fallbackOn = false;
			sDecodingFallback fallbackParams;
			std::vector<sWindowStats> windowStats;
			// Whisper::setSuppressedTokens: empty unless set; every device context this object owns holds it (beamContext tells the ones created later)
			std::vector<int32_t> suppressIds;
			// Whisper::setTimestampRules: off unless set. The stream's device context holds the mode; the hypothesis-group context of beam search cannot (runFull refuses)
			bool timestampRulesOn = false;
			// Whisper::setBoostedPhrases: off unless set. The stream's device context holds the set; the hypothesis-group context of beam search cannot (runFull refuses)
			bool boostOn = false;
			// Whisper::setNoRepeatNgram: 0 = off unless set. The stream's device context holds n; the hypothesis-group context of beam search cannot (runFull refuses)
			int noRepeatN = 0;
			// Whisper::setSpeechFilter: off unless set. A run with it on packs the speech of the uploaded PCM on the device (wh_context_speech_filter) and works on the
			// packed buffer; runSpans / runMap are what the last run used (the map is empty when the run's clock is the recording's)
			bool speechOn = false;
			sSpeechFilter speechParams{};
			std::vector<speechRules::Span> runSpans;
			speechRules::TimeMap runMap;
			// the filter on the context's resident PCM (pcmDev, n samples). packed: what the spectrogram is taken from -- pcmDev itself when one span covers it all,
			// nullptr when there is no speech
			HRESULT filterSpeech( int64_t n, const float*& packed, int64_t& nPacked )
			{
				runSpans.clear();
				runMap = speechRules::TimeMap{};
				const wh_speech_params p{ speechParams.minSilenceFrames, speechParams.minSpeechFrames, speechParams.padFrames };
				// the spans of a recording are at least a frame long and a frame apart
				const int cap = (int)std::min<int64_t>( 65536, n / ( 2 * vad::FRAME_SAMPLES ) + 1 );
				std::vector<int64_t> flat( (size_t)cap * 2 );
				int count = 0;
				CHECK_WH( wh_context_speech_filter( gpu, (const float*)pcmDev, n, nullptr, &p, &packed, nullptr, &nPacked, flat.data(), cap, &count ) );
				for( int i = 0; i < count; i++ ) runSpans.push_back( speechRules::Span{ flat[ (size_t)i * 2 ], flat[ (size_t)i * 2 + 1 ] } );
				if( count > 0 && !speechRules::coversAll( runSpans, n ) ) runMap.assign( runSpans );
				return S_OK;
			}
			// what a run with the filter on refuses
			HRESULT speechFilterAccepts( const char* who, const sFullParams& params ) const
			{
				if( params.offset_ms != 0 || params.duration_ms != 0 )
				{
					logError( "%s: offset_ms and duration_ms are not available with the speech filter (setSpeechFilter) on", who );
					return E_INVALIDARG;
				}
				if( params.flag( eFullParamsFlags::TokenTimestamps ) )
				{
					logError( "%s: eFullParamsFlags::TokenTimestamps is not available with the speech filter (setSpeechFilter) on: its stamper reads the host's PCM", who );
					return E_NOTIMPL;
				}
				return S_OK;
			}
			// no speech at all: S_OK, no segments, nothing encoded
			HRESULT nothingToTranscribe( const char* who, int64_t n )
			{
				logInfo( "%s: the speech filter found no speech in %.2f s of audio; nothing to transcribe", who, (double)n / 16000.0 );
				resultAll.clear();
				speakers.clear();
				windowStats.clear();
				detectedLang = -1;
				detectedP = 0;
				return S_OK;
			}

			using Clock = std::chrono::steady_clock;
			static double msSince( Clock::time_point t ) { return std::chrono::duration<double, std::milli>( Clock::now() - t ).count(); }

			// iSpectrogram of the reference: runFull hands the loop a whole-buffer spectrogram (global maximum), runStreamed a
			// MelStreamer that makes each window on demand with the window's own maximum (MelStreamer.cpp:125-245)
			struct MelSource
			{
				bool streamed = false;
				int64_t length = 0;			  // iSpectrogram::getLength(): 10 ms frames
				int64_t nSamples = 0, nChunks = 0;
				int64_t lastBufferEnd = -1;	  // MelStreamer::lastBufferEnd
				const float* pcm = nullptr;	  // streamed: the resident samples the windows are taken from (the context's PCM buffer, or its packed speech)
			};
			MelSource mel;

			HRESULT ensureBuffer( void*& dev, int64_t& cap, int64_t bytes )
			{
				CHECK_WH( wh_context_bind( gpu ) );
				if( bytes <= cap ) return S_OK;
				if( dev ) { wh_buffer_free( dev ); dev = nullptr; cap = 0; }
				CHECK_WH( wh_buffer_alloc( bytes, &dev ) );
				cap = bytes;
				return S_OK;
			}
			HRESULT fillResults( eResultFlags flags, ResultData& res ) const;
			HRESULT runFullImpl( const sFullParams& params, const sProgressSink& progress );
			HRESULT encodeWindow( wh_context* ctx, int seek );
			int audioCtx = 0;	   // sFullParams::audio_ctx of the run in progress (0 = the model's)
			HRESULT beamContext( int width );
			HRESULT activeContext( const sFullParams& params, bool warn, wh_context*& active, int& beamWidth );
			// language "auto" (languageDetect.h): what the last run / detectLanguage call found, -1 = nothing was detected
			int detectedLang = -1;
			float detectedP = 0;
			HRESULT detectOnWindow( wh_context* ctx, int seek, std::vector<float>* probs, int& langId );
			HRESULT resolveLanguage( sFullParams& params, bool& firstWindowEncoded );
			HRESULT decodeWindowBeam( const std::vector<int>& prompt, int width, WindowScan& scan, int& steps );
			HRESULT decodeWindowBeamDevice( const std::vector<int>& prompt, int width, WindowScan& scan, int& steps );

		public:
			ContextImpl( const std::shared_ptr<LoadedModel>& m, iModel* o ) : model( m ), owner( o )
			{
				if( owner ) owner->AddRef();
			}
			~ContextImpl() override
			{
				if( gpu ) wh_context_bind( gpu );
				if( melDev ) wh_buffer_free( melDev );
				if( pcmDev ) wh_buffer_free( pcmDev );
				if( gpuBeam ) wh_context_destroy( gpuBeam );
				if( gpu ) wh_context_destroy( gpu );
				if( owner ) owner->Release();
			}
			HRESULT init()
			{
				CHECK_WH( wh_context_create( model->gpu, 1, nullptr, &gpu ) );
				// The reference profiles every dispatch all the time (GpuProfiler). Here the event pairs force eager launches
				// (no hipGraph replay), so the per-kernel table is opt-in.
				const char* const env = getenv( "WHISPER_PROFILE" );
				gpuProfile = env && env[ 0 ] && env[ 0 ] != '0';
				if( gpuProfile ) CHECK_WH( wh_profile_enable( gpu, 1 ) );
				return S_OK;
			}

			// whisper_lang_auto_detect on a buffer of its own (whisperc_detect_language), and the language of the last run
			HRESULT detectLanguage( const float* pcm, uint32_t nSamples, int offsetMs, float* probs, uint32_t probsCap, int& langId );
			int lastDetectedLanguage( float& p ) const { p = detectedP; return detectedLang; }
			// wh_context_set_flags on this context's device context (whisperc_debug_context_flags: the exact mode for parity tests)
			HRESULT setDeviceFlags( uint32_t flags, int parityThreads )
			{
				CHECK_WH( wh_context_set_flags( gpu, flags, parityThreads ) );
				return S_OK;
			}
			HRESULT setFallback( const sDecodingFallback* p )
			{
				if( !p ) { fallbackOn = false; return S_OK; }
				CHECK( optionRules::checkFallback( "setDecodingFallback", *p ) );
				fallbackParams = *p;
				fallbackOn = true;
				return S_OK;
			}
			HRESULT setSuppressed( const int32_t* ids, uint32_t count )
			{
				CHECK( optionRules::checkSuppressed( "setSuppressedTokens", ids, count, model->vocab.token_eot ) );
				CHECK_WH( wh_context_set_suppress( gpu, ids, (int)count ) );
				if( gpuBeam ) CHECK_WH( wh_context_set_suppress( gpuBeam, ids, (int)count ) );
				suppressIds.assign( ids, ids + count );
				return S_OK;
			}
			// Whisper::scoreTokens: the clip's spectrogram (normalised on its own maximum, like runFull's of those samples), one window at seek 0 with the model's
			// full audio context, then the teacher-forced pass; frames != nullptr: the same row through wh_align_tokens with the keys runFull's aligner takes
			HRESULT scoreClip( const float* pcm, int64_t n, const int32_t* tokens, int32_t len, int32_t firstScored, wh_token_score* recs, int32_t* frames )
			{
				const wh_hparams& hp = model->hp;
				const int64_t melLen = n / 160;
				mel = MelSource{};
				mel.length = melLen;
				CHECK( ensureBuffer( pcmDev, pcmCapacity, n * 4 ) );
				CHECK( ensureBuffer( melDev, melCapacity, melLen * hp.n_mels * 4 ) );
				CHECK_WH( wh_buffer_upload( gpu, pcmDev, pcm, n * 4 ) );
				int64_t got = 0;
				CHECK_WH( wh_mel_spectrogram( gpu, (const float*)pcmDev, n, (float*)melDev, &got ) );
				audioCtx = 0;
				CHECK_WH( wh_context_set_audio_ctx( gpu, 0 ) );
				const int32_t off = 0;
				CHECK_WH( wh_encode( gpu, (const float*)melDev, 1, melLen, melLen * hp.n_mels, &off ) );
				CHECK_WH( wh_score_tokens( gpu, 1, tokens, &len, &firstScored, len, recs ) );
				if( frames )
				{
					const int32_t nKeys = (int32_t)std::max<int64_t>( 1, std::min<int64_t>( hp.n_audio_ctx, melLen / 2 ) );
					CHECK_WH( wh_align_tokens( gpu, 1, tokens, &len, &nKeys, len, frames ) );
				}
				return S_OK;
			}
			HRESULT setTimestampRulesMode( bool on )
			{
				CHECK_WH( wh_context_set_timestamp_rules( gpu, on ? 1 : 0 ) );
				timestampRulesOn = on;
				return S_OK;
			}
			HRESULT setSpeech( const sSpeechFilter* p )
			{
				if( !p ) { speechOn = false; return S_OK; }
				CHECK( optionRules::checkSpeechFilter( "setSpeechFilter", *p ) );
				speechParams = *p;
				speechOn = true;
				return S_OK;
			}
			const std::vector<speechRules::Span>& lastSpeechSpans() const { return runSpans; }
			HRESULT setNoRepeat( int n )
			{
				CHECK( optionRules::checkNoRepeat( "setNoRepeatNgram", n ) );
				CHECK_WH( wh_context_set_no_repeat( gpu, n ) );
				noRepeatN = n;
				return S_OK;
			}
			HRESULT setBoosted( const sBoostedPhrases* p )
			{
				phraseBoost::Set set;
				CHECK( optionRules::checkBoosted( "setBoostedPhrases", p, model->vocab.token_eot, set ) );
				CHECK_WH( wh_context_set_boost( gpu, set.tokens.data(), set.lens.data(), set.count(), set.nMax, set.boost ) );
				boostOn = set.count() > 0;
				return S_OK;
			}
			const std::vector<sWindowStats>& lastWindowStats() const { return windowStats; }
			HRESULT runFull( const sFullParams& params, const iAudioBuffer* buffer ) override;
			HRESULT runStreamed( const sFullParams& params, const sProgressSink& progress, const iAudioReader* reader ) override;
			// capture.cpp: the reference's capture loop over an iPcmCapture, every piece a runFull of this context on a worker thread
			HRESULT runCapture( const sFullParams& params, const sCaptureCallbacks& callbacks, const iAudioCapture* reader ) override
			{
				return runCapturePieces( params, callbacks, reader, nullptr, nullptr );
			}
			HRESULT runCapturePieces( const sFullParams& params, const sCaptureCallbacks& callbacks, const iAudioCapture* reader, pfnCapturePiece pfnPiece, void* pvPiece )
			{
				// the speech filter does not apply to a capture: its pieces are fired by the same detector already. Off while the loop runs its runFull calls
				struct FilterOff
				{
					bool& on;
					const bool was;
					explicit FilterOff( bool& b ) : on( b ), was( b ) { on = false; }
					~FilterOff() { on = was; }
				} filterOff( speechOn );
				return runCaptureLoop( this, gpu, params, callbacks, reader, pfnPiece, pvPiece );
			}
			HRESULT getResults( eResultFlags flags, iTranscribeResult** pp ) const override;
			HRESULT detectSpeaker( const sTimeInterval& time, eSpeakerChannel& result ) const override
			{
				if( !runCurrent )
				{
					logError( "Because the audio is streamed, iContext.detectSpeaker() method only works when called from the callbacks" );
					return OLE_E_BLANK;
				}
				return diarize::detectSpeaker( stereoPcm, stereoFrames, mediaTimeOffset, time, result );
			}
			HRESULT getModel( iModel** pp ) override
			{
				if( !pp ) return E_POINTER;
				if( !owner ) return E_UNEXPECTED;
				owner->AddRef();
				*pp = owner;
				return S_OK;
			}
			HRESULT fullDefaultParams( eSamplingStrategy strategy, sFullParams* rdi ) override { return defaultFullParams( strategy, rdi ); }
			HRESULT timingsPrint() override;
			HRESULT timingsReset() override
			{
				msSpectrogram = msEncode = msDecode = msRun = 0;
				nEncode = nDecodeSteps = nRuns = nSpectrogram = nDecodeWindows = 0;
				if( gpuProfile ) wh_profile_enable( gpu, 1 );
				return S_OK;
			}
		};

		HRESULT ContextImpl::timingsPrint()
		{
			// Sections, block names and line format of the reference's profiler output (ProfileCollection::print,
			// ContextImpl.misc.cpp:170-182, e.g. SampleClips/columbia-medium-1080ti.txt) so that logs stay comparable.
			constexpr double ticksPerMs = 1.0e4;
			logInfo( "    CPU Tasks" );
			if( nRuns ) logInfo( "%s", formatMeasure( "RunComplete", msRun * ticksPerMs, nRuns ).c_str() );
			if( nSpectrogram ) logInfo( "%s", formatMeasure( "Spectrogram", msSpectrogram * ticksPerMs, nSpectrogram ).c_str() );
			if( nEncode ) logInfo( "%s", formatMeasure( "Encode", msEncode * ticksPerMs, nEncode ).c_str() );
			if( nDecodeWindows ) logInfo( "%s", formatMeasure( "Decode", msDecode * ticksPerMs, nDecodeWindows ).c_str() );
			if( nDecodeSteps ) logInfo( "%s", formatMeasure( "DecodeStep", msDecode * ticksPerMs, nDecodeSteps ).c_str() );
			if( gpuProfile )
			{
				// one row per kernel class, longest first -- the "Compute Shaders" table of the reference
				wh_profile_entry rows[ 32 ];
				int n = 0;
				if( 0 == wh_profile_read( gpu, rows, 32, &n ) && n > 0 )
				{
					std::sort( rows, rows + n, []( const wh_profile_entry& a, const wh_profile_entry& b ) { return a.ms > b.ms; } );
					logInfo( "    Compute Shaders" );
					for( int i = 0; i < n; i++ )
						if( rows[ i ].calls > 0 ) logInfo( "%s", formatMeasure( rows[ i ].name, rows[ i ].ms * ticksPerMs, (uint64_t)rows[ i ].calls ).c_str() );
				}
			}
			int64_t ctxVram = 0, modelVram = 0;
			void* arena = nullptr;
			wh_context_memory( gpu, &ctxVram );
			wh_model_arena( model->gpu, &arena, &modelVram );
			int64_t modelRam = 0;
			for( const std::string& t : model->vocab.idToToken ) modelRam += (int64_t)t.size() * 2 + 2 * (int64_t)sizeof( std::string );
			const int64_t ctxRam = (int64_t)( resultAll.capacity() * sizeof( Segment ) + promptPast.capacity() * sizeof( int ) );
			logInfo( "    Memory Usage" );
			logInfo( "Model\t%s RAM, %s VRAM", formatBytes( (double)modelRam ).c_str(), formatBytes( (double)modelVram ).c_str() );
			logInfo( "Context\t%s RAM, %s VRAM", formatBytes( (double)ctxRam ).c_str(), formatBytes( (double)ctxVram ).c_str() );
			logInfo( "Total\t%s RAM, %s VRAM", formatBytes( (double)( modelRam + ctxRam ) ).c_str(), formatBytes( (double)( modelVram + ctxVram ) ).c_str() );
			return S_OK;
		}

		HRESULT ContextImpl::runFull( const sFullParams& params, const iAudioBuffer* buffer )
		{
			if( !buffer ) return E_POINTER;
			if( speechOn ) CHECK( speechFilterAccepts( "runFull", params ) );
			const auto tRun = Clock::now();
			CHECK( buffer->getTime( mediaTimeOffset ) );
			const uint32_t n = buffer->countSamples();
			const float* pcm = buffer->getPcmMono();
			int64_t melLen = n / 160;
			mel = MelSource{};
			mel.length = melLen;
			stereoPcm = buffer->getPcmStereo();	   // a foreign buffer without stereo data: nullptr, NoStereoData
			stereoFrames = stereoPcm ? n : 0;
			runSpans.clear();
			runMap = speechRules::TimeMap{};
			if( melLen > 0 )
			{
				const auto t = Clock::now();
				CHECK( ensureBuffer( pcmDev, pcmCapacity, (int64_t)n * 4 ) );
				CHECK_WH( wh_buffer_upload( gpu, pcmDev, pcm, (int64_t)n * 4 ) );
				// speech only: the spectrogram of the packed speech instead of the recording's; the loop below never learns the difference
				const float* source = (const float*)pcmDev;
				int64_t nSource = n;
				if( speechOn )
				{
					CHECK( filterSpeech( n, source, nSource ) );
					if( !source )
					{
						stereoPcm = nullptr;
						stereoFrames = 0;
						return nothingToTranscribe( "runFull", n );
					}
					mel.length = melLen = nSource / 160;
				}
				if( melLen > 0 )
				{
					CHECK( ensureBuffer( melDev, melCapacity, melLen * model->hp.n_mels * 4 ) );
					int64_t got = 0;
					CHECK_WH( wh_mel_spectrogram( gpu, source, nSource, (float*)melDev, &got ) );
					CHECK_WH( wh_context_synchronize( gpu ) );
				}
				msSpectrogram += msSince( t );
				nSpectrogram++;
			}
			else if( speechOn )
			{
				stereoPcm = nullptr;
				stereoFrames = 0;
				return nothingToTranscribe( "runFull", n );
			}
			if( params.flag( eFullParamsFlags::TokenTimestamps ) ) stamper.begin( pcm, n );
			const sProgressSink noProgress{ nullptr, nullptr };
			const HRESULT hr = runFullImpl( params, noProgress );
			msRun += msSince( tRun );
			nRuns++;
			return hr;
		}

		// ContextImpl::runStreamed (Whisper/Whisper/ContextImpl.misc.cpp:391-419): the same loop over a spectrogram that is
		// made window by window. What differs from runFull in the RESULTS is the normalisation: every window is clamped
		// against its own maximum (floor 1e-20, FP32 arithmetic) instead of the whole recording's, and a request that ends
		// where the previous one ended re-uses the previous maximum (MelStreamer.cpp:148-166). The PCM of the reader is
		// resident in HBM (a 3 h recording is 690 MB of 288 GB); only the window's frames are ever transformed.
		HRESULT ContextImpl::runStreamed( const sFullParams& params, const sProgressSink& progress, const iAudioReader* reader )
		{
			if( !reader ) return E_POINTER;
			if( params.flag( eFullParamsFlags::TokenTimestamps ) )
			{
				logError( "eFullParamsFlags.TokenTimestamps flag is not supported in streaming mode" );
				return E_NOTIMPL;
			}
			if( speechOn ) CHECK( speechFilterAccepts( "runStreamed", params ) );
			iPcmSource* src = nullptr;
			if( FAILED( const_cast<iAudioReader*>( reader )->QueryInterface( iPcmSource::iid(), (void**)&src ) ) || !src )
			{
				logError( "runStreamed: this reader was not created by iMediaFoundation::openAudioFile / loadAudioFileData of this library" );
				return E_INVALIDARG;
			}
			const auto tRun = Clock::now();
			mediaTimeOffset = 0;
			const std::vector<float>& pcm = src->pcmMono();
			mel = MelSource{};
			mel.streamed = true;
			mel.nSamples = (int64_t)pcm.size();
			mel.length = mel.nSamples / 160;			   // PcmReader::getLength(): whole 10 ms chunks (PcmReader.h:50-55)
			mel.nChunks = ( mel.nSamples + 159 ) / 160;	   // readChunk pads the last incomplete chunk with zeros (PcmReader.cpp:416-424)
			// The reference's MelStreamer keeps the stereo chunks of the current window only and answers E_UNEXPECTED for times behind it
			// (MelStreamer.cpp:495-534); the whole recording is resident here, so those times are answered too.
			const std::vector<float>& st = src->pcmStereo();
			stereoFrames = std::min( st.size() / 2, pcm.size() );
			stereoPcm = stereoFrames ? st.data() : nullptr;
			HRESULT hr = S_OK;
			runSpans.clear();
			runMap = speechRules::TimeMap{};
			mel.pcm = nullptr;
			bool noSpeech = false;
			if( mel.nSamples > 0 )
			{
				hr = ensureBuffer( pcmDev, pcmCapacity, mel.nSamples * 4 );
				if( SUCCEEDED( hr ) ) hr = ensureBuffer( melDev, melCapacity, (int64_t)std::max( CHUNK_FRAMES, 2 * model->hp.n_audio_ctx ) * model->hp.n_mels * 4 );	// encodeWindow asks for up to 2 * n_audio_ctx frames
				if( SUCCEEDED( hr ) && 0 != wh_buffer_upload( gpu, pcmDev, pcm.data(), mel.nSamples * 4 ) ) hr = E_FAIL;
				mel.pcm = (const float*)pcmDev;
				// speech only: the resident PCM is packed once, the windows are taken from the packed buffer and progress counts its frames
				if( SUCCEEDED( hr ) && speechOn )
				{
					const float* packed = nullptr;
					int64_t nPacked = 0;
					hr = filterSpeech( mel.nSamples, packed, nPacked );
					if( SUCCEEDED( hr ) )
					{
						noSpeech = !packed;
						mel.pcm = packed;
						mel.nSamples = nPacked;
						mel.length = nPacked / 160;
						mel.nChunks = ( nPacked + 159 ) / 160;
					}
				}
			}
			else if( speechOn ) noSpeech = true;
			if( SUCCEEDED( hr ) && noSpeech )
			{
				stereoPcm = nullptr;
				stereoFrames = 0;
				hr = nothingToTranscribe( "runStreamed", (int64_t)pcm.size() );
			}
			else if( SUCCEEDED( hr ) ) hr = runFullImpl( params, progress );
			src->Release();
			msRun += msSince( tRun );
			nRuns++;
			return hr;
		}

		// ContextImpl::encode( iSpectrogram&, seek ) + MelInputTensor::create (MelInputTensor.cpp:8-63)
		HRESULT ContextImpl::encodeWindow( wh_context* gpu, int seek )
		{
			const wh_hparams& hp = model->hp;
			if( !mel.streamed )
			{
				const int32_t off = seek;
				CHECK_WH( wh_encode( gpu, (const float*)melDev, 1, mel.length, mel.length * hp.n_mels, &off ) );
				return S_OK;
			}
			const int64_t i0 = std::min( (int64_t)seek, mel.length );
			const int64_t i1 = std::min( (int64_t)seek + 2 * ( audioCtx > 0 ? audioCtx : hp.n_audio_ctx ), mel.length );
			if( i1 <= i0 ) return E_BOUNDS;
			const auto t = Clock::now();
			const bool reuse = mel.lastBufferEnd == i1;
			CHECK_WH( wh_mel_spectrogram_window( gpu, mel.pcm, mel.nSamples, i0, i1 - i0, mel.nChunks, reuse ? 1 : 0, (float*)melDev ) );
			if( !reuse ) mel.lastBufferEnd = i1;
			msSpectrogram += msSince( t );	   // enqueue time only: the transform overlaps nothing else and is < 1 % of a window
			nSpectrogram++;
			const int32_t zero = 0;
			CHECK_WH( wh_encode( gpu, (const float*)melDev, 1, i1 - i0, ( i1 - i0 ) * hp.n_mels, &zero ) );
			return S_OK;
		}

		// The token stream of one window. The prompt step, the first sample (sampleTimestamp(true) of the reference) and the
		// first chunk of greedy steps are enqueued at once; the host then reads chunk k while chunk k+1 runs and, if no stop
		// rule fired on chunk k, enqueues chunk k+2 before it waits for k+1 -- the device never waits for the host, and one
		// chunk (GREEDY_CHUNK steps) is decoded in vain when a window ends.
		class WindowDecoder
		{
			wh_context* gpu;
			int nTextCtx, nPrompt = 0;
			int enqueued = 0;	  // samples enqueued so far (1 + greedy steps)
			int fetched = 0;	  // samples copied to `buf`
			std::vector<wh_token_data> buf;
			size_t cursor = 0;
			int room() const { return nTextCtx - ( nPrompt + enqueued - 1 ); }	// positions left for further greedy steps
			HRESULT enqueueChunk()
			{
				const int n = std::min( GREEDY_CHUNK, room() );
				if( n <= 0 ) return S_FALSE;
				CHECK_WH( wh_decode_window_continue( gpu, n ) );
				enqueued += n;
				return S_OK;
			}
		public:
			int steps = 0;
			double msFetch = 0, msEnqueue = 0;	   // host time waiting for samples / enqueueing further steps (WHISPER_HOSTPROF)
			WindowDecoder( wh_context* c, int nTextCtx_ ) : gpu( c ), nTextCtx( nTextCtx_ ) {}
			HRESULT start( const std::vector<int>& prompt, TokenData& first )
			{
				nPrompt = (int)prompt.size();
				const int n0 = std::max( 0, std::min( GREEDY_CHUNK, nTextCtx - nPrompt ) );
				CHECK_WH( wh_decode_window_start( gpu, 1, prompt.data(), nPrompt, n0, 1, 1 ) );
				enqueued = 1 + n0;
				buf.resize( 1 );
				CHECK_WH( wh_decode_window_fetch( gpu, 0, 1, buf.data() ) );
				fetched = 1;
				cursor = 1;
				const wh_token_data& t = buf[ 0 ];
				first.id = t.id; first.tid = t.tid; first.p = t.p; first.pt = t.pt; first.ptsum = t.ptsum;
				steps = 1;
				return S_OK;
			}
			HRESULT next( TokenData& out )
			{
				if( cursor >= buf.size() )
				{
					// The caller has looked at everything handed out so far and wants more: NOW the chunk after the one in flight is
					// queued (the one in flight has been running since the previous fetch returned, so the device does not wait
					// for this), then the chunk in flight is awaited. A window that ends on the token just examined therefore
					// leaves ONE chunk decoded in vain, not two.
					const auto t0 = std::chrono::steady_clock::now();
					CHECK( enqueueChunk() );
					const auto t1 = std::chrono::steady_clock::now();
					if( fetched >= enqueued ) return E_BOUNDS;
					// the chunk that follows what has been read: everything up to the next chunk boundary
					const int n = std::min( GREEDY_CHUNK, enqueued - fetched );
					buf.resize( (size_t)n );
					CHECK_WH( wh_decode_window_fetch( gpu, fetched, n, buf.data() ) );
					fetched += n;
					cursor = 0;
					msEnqueue += std::chrono::duration<double, std::milli>( t1 - t0 ).count();
					msFetch += std::chrono::duration<double, std::milli>( std::chrono::steady_clock::now() - t1 ).count();
				}
				const wh_token_data& t = buf[ cursor++ ];
				out.id = t.id; out.tid = t.tid; out.p = t.p; out.pt = t.pt; out.ptsum = t.ptsum;
				steps++;
				return S_OK;
			}
		};

		// A context of one window x `slots` hypotheses (1, 2, 3, 4, 5 or 8 per window: wh_context_create_hyp)
		HRESULT ContextImpl::beamContext( int width )
		{
			const int slots = width <= 5 ? width : 8;
			if( gpuBeam && beamSlots == slots ) return S_OK;
			if( gpuBeam ) { wh_context_destroy( gpuBeam ); gpuBeam = nullptr; }
			CHECK_WH( wh_context_create_hyp( model->gpu, 1, slots, nullptr, &gpuBeam ) );
			beamSlots = slots;
			if( !suppressIds.empty() ) CHECK_WH( wh_context_set_suppress( gpuBeam, suppressIds.data(), (int)suppressIds.size() ) );
			return S_OK;
		}

		// Beam search over one window (extension; the reference only declares the strategy). `width` hypotheses decode in lock step and
		// share the window's cross-attention K/V (wh_context_create_hyp). A step: every live hypothesis proposes its `width` best
		// continuations under sampleBest's own rules (wh_beam_candidates: candidate 0 is the greedy token), the pool is ranked by
		// cumulative log-probability, the best `width` survive -- each either stays live (its parent's self-attention cache rows are
		// copied into its slot, wh_reorder_self_cache) or, when the reference's stop rules end its window (WindowScan: EOT, a timestamp
		// that goes back, end of audio, max_tokens ...), joins the finished list. The window's transcript is the finished hypothesis with
		// the best log-probability per token; hypotheses the stop rules call failed count only if nothing else finished.
		// Width 1 is the greedy decoder token for token (tests/test_host_api.py::test_beam_search).
		HRESULT ContextImpl::decodeWindowBeam( const std::vector<int>& prompt, int width, WindowScan& result, int& steps )
		{
			const int B = beamSlots, n = (int)prompt.size();
			struct Hyp
			{
				std::unique_ptr<WindowScan> scan;
				double sum = 0.0;
				int slot = 0;
			};
			std::vector<Hyp> live, finished;
			std::vector<int32_t> tokens( (size_t)B * std::max( n, 1 ) ), parents( (size_t)B, 0 ), next( (size_t)B, 0 );
			for( int b = 0; b < B; b++ ) std::copy( prompt.begin(), prompt.end(), tokens.begin() + (size_t)b * n );
			CHECK_WH( wh_decode( gpuBeam, tokens.data(), B, n, 0, nullptr, nullptr ) );
			std::vector<wh_token_data> cand( (size_t)B * width );
			CHECK_WH( wh_beam_candidates( gpuBeam, B, width, 1, 1, cand.data() ) );
			steps = 1;
			// what a parent proposes: (parent index in `live`, candidate) ranked by parent score + log p; ties keep the parent's order
			struct Prop { int parent, k; double score; };
			auto expand = [ & ]( const std::vector<Hyp>& parentsHyp, const std::vector<Prop>& pool, std::vector<Hyp>& newLive )
			{
				int accepted = 0;
				for( const Prop& pr : pool )
				{
					if( accepted >= width ) break;
					const Hyp& par = parentsHyp[ (size_t)pr.parent ];
					const wh_token_data& t = cand[ (size_t)par.slot * width + pr.k ];
					Hyp h;
					h.scan.reset( new WindowScan( *par.scan ) );
					h.sum = pr.score;
					h.slot = par.slot;	 // its cache rows live in the parent's slot until the reorder
					TokenData td;
					td.id = t.id; td.tid = t.tid; td.p = t.p; td.pt = t.pt; td.ptsum = t.ptsum;
					const bool over = h.scan->feed( td );
					accepted++;
					if( over ) finished.push_back( std::move( h ) );
					else newLive.push_back( std::move( h ) );
				}
			};
			{
				// the first sample: every slot holds the same prompt, slot 0 speaks for all
				std::vector<Hyp> root( 1 );
				root[ 0 ].scan.reset( new WindowScan( result ) );
				root[ 0 ].slot = 0;
				std::vector<Prop> pool;
				for( int k = 0; k < width; k++ ) pool.push_back( Prop{ 0, k, log( std::max( (double)cand[ (size_t)k ].p, 1e-30 ) ) } );
				std::stable_sort( pool.begin(), pool.end(), []( const Prop& a, const Prop& b ) { return a.score > b.score; } );
				expand( root, pool, live );
			}
			// The search goes on while a live hypothesis could still win: a finished list that is full ends it only once every live
			// hypothesis has fallen below the best finished one (a cumulative log-probability only ever decreases). Low-probability
			// continuations that end their window at once (an EOT proposed with p ~ 1e-5) fill the list early and must not stop the
			// hypothesis that is still being transcribed.
			auto keepSearching = [ & ]() -> bool
			{
				if( live.empty() ) return false;
				if( (int)finished.size() < width ) return true;
				double bestFinished = -1e300, bestLive = -1e300;
				for( const Hyp& h : finished )
					if( !h.scan->failed ) bestFinished = std::max( bestFinished, h.sum );
				for( const Hyp& h : live ) bestLive = std::max( bestLive, h.sum );
				return bestLive >= bestFinished;
			};
			auto perToken = []( const Hyp& h ) { return h.sum / (double)std::max<size_t>( 1, h.scan->tokens.size() ); };
			for( int s = 0; keepSearching(); s++ )
			{
				// the finished list keeps its best `width` entries (successful windows first, then log-probability per token)
				if( (int)finished.size() > 2 * width )
				{
					std::stable_sort( finished.begin(), finished.end(), [ & ]( const Hyp& a, const Hyp& b )
						{ return a.scan->failed != b.scan->failed ? !a.scan->failed : perToken( a ) > perToken( b ); } );
					finished.resize( (size_t)width );
				}
				if( n + s >= model->hp.n_text_ctx ) break;	   // WindowScan's own bound (n_text_ctx / 2 - 4 tokens) fires first for every prompt the loop builds
				// live hypothesis i moves to slot i; the idle slots repeat slot 0 and are ignored
				for( int b = 0; b < B; b++ )
				{
					const Hyp& h = live[ (size_t)( b < (int)live.size() ? b : 0 ) ];
					parents[ (size_t)b ] = h.slot;
					next[ (size_t)b ] = h.scan->tokens.back().id;
				}
				// a hypothesis that stopped on a token WindowScan did not keep (a timestamp going back) never reaches this point: it is finished
				CHECK_WH( wh_reorder_self_cache( gpuBeam, B, parents.data(), n + s ) );
				for( size_t i = 0; i < live.size(); i++ ) live[ i ].slot = (int)i;
				CHECK_WH( wh_decode( gpuBeam, next.data(), B, 1, n + s, nullptr, nullptr ) );
				CHECK_WH( wh_beam_candidates( gpuBeam, B, width, 0, 0, cand.data() ) );
				steps++;
				std::vector<Prop> pool;
				for( int i = 0; i < (int)live.size(); i++ )
					for( int k = 0; k < width; k++ )
						pool.push_back( Prop{ i, k, live[ (size_t)i ].sum + log( std::max( (double)cand[ (size_t)live[ (size_t)i ].slot * width + k ].p, 1e-30 ) ) } );
				std::stable_sort( pool.begin(), pool.end(), []( const Prop& a, const Prop& b ) { return a.score > b.score; } );
				std::vector<Hyp> newLive;
				expand( live, pool, newLive );
				live = std::move( newLive );
			}
			// hypotheses still live when the list filled up (or the context ran out) are candidates too: they end where they stand, as failed
			// windows do when the loop's bound is reached
			for( Hyp& h : live )
			{
				if( !h.scan->over ) h.scan->failed = h.scan->over = true;
				finished.push_back( std::move( h ) );
			}
			const Hyp* best = nullptr;
			for( const Hyp& h : finished )
				if( !best || ( best->scan->failed && !h.scan->failed ) || ( best->scan->failed == h.scan->failed && perToken( h ) > perToken( *best ) ) ) best = &h;
			if( !best ) return E_UNEXPECTED;
			result.adopt( *best->scan );
			return S_OK;
		}

		// The same search with the ranking ON THE DEVICE (round 5): wh_beam_window_* keeps pool, ranking, stop rules, finished / live lists and the
		// "can a live hypothesis still win" test in a kernel behind every decode step, the whole step is one captured graph, and this loop only polls
		// `done` every 16 steps -- a window of ~50 tokens costs 4 host round trips instead of 100. What comes back: the search state (who finished with
		// which score) and one record per accepted proposal; the winner is chosen by decodeWindowBeam's own rule and its tokens are REPLAYED through the
		// window's WindowScan, which both builds the result and checks the device's restatement of the stop rules against the host's.
		HRESULT ContextImpl::decodeWindowBeamDevice( const std::vector<int>& prompt, int width, WindowScan& result, int& steps )
		{
			const int n = (int)prompt.size(), nCtx = model->hp.n_text_ctx;
			wh_beam_rules rules{};
			bool single = false;
			{
				int seek = 0, seekEnd = 0, nMax = 0, maxTokens = 0;
				result.constants( seek, seekEnd, nMax, maxTokens, single );
				rules.seek = seek; rules.seekEnd = seekEnd; rules.nMax = nMax; rules.maxTokens = maxTokens;
			}
			rules.singleSegment = single ? 1 : 0;
			rules.tokenBeg = model->vocab.token_beg;
			rules.tokenEot = model->vocab.token_eot;
			rules.forced = 0;
			constexpr int CHUNK = 16;
			int enqueued = std::max( 0, std::min( CHUNK - 1, nCtx - n ) );
			std::vector<int32_t> tokens( prompt.begin(), prompt.end() );
			CHECK_WH( wh_beam_window_start( gpuBeam, 1, tokens.data(), n, width, &rules, enqueued ) );
			wh_beam_window st{};
			while( true )
			{
				CHECK_WH( wh_beam_window_status( gpuBeam, &st ) );
				if( st.done ) break;
				const int more = std::min( CHUNK, nCtx - n - enqueued );
				if( more <= 0 ) break;
				CHECK_WH( wh_beam_window_continue( gpuBeam, more ) );
				enqueued += more;
			}
			steps = st.step;
			if( st.step <= 0 ) return E_UNEXPECTED;
			std::vector<wh_beam_record> rec( (size_t)st.step * width );
			CHECK_WH( wh_beam_window_records( gpuBeam, 0, st.step, rec.data() ) );
			// the candidates in decodeWindowBeam's order: the finished list, then whoever was still live (those end where they stand, as failed windows)
			struct Cand { wh_beam_hyp h; bool wasLive; };
			std::vector<Cand> cands;
			for( int i = 0; i < st.nFinished; i++ ) cands.push_back( Cand{ st.finished[ i ], false } );
			for( int i = 0; i < st.nLive; i++ )
			{
				Cand c{ st.live[ i ], true };
				if( !c.h.over ) c.h.failed = c.h.over = 1;
				cands.push_back( c );
			}
			auto perToken = []( const wh_beam_hyp& h ) { return h.sum / (double)std::max( 1, h.nTok ); };
			const Cand* best = nullptr;
			for( const Cand& c : cands )
				if( !best || ( best->h.failed && !c.h.failed ) || ( ( best->h.failed != 0 ) == ( c.h.failed != 0 ) && perToken( c.h ) > perToken( best->h ) ) ) best = &c;
			if( !best ) return E_UNEXPECTED;
			// its tokens, oldest first
			std::vector<const wh_beam_record*> chain;
			for( int r = best->h.rec; r >= 0; )
			{
				if( r >= st.step * width ) return E_UNEXPECTED;
				const wh_beam_record& x = rec[ (size_t)r ];
				chain.push_back( &x );
				r = x.parent;
			}
			WindowScan replay( result );
			for( size_t k = chain.size(); k-- > 0; )
			{
				const wh_beam_record& x = *chain[ k ];
				TokenData td;
				td.id = x.t.id; td.tid = x.t.tid; td.p = x.t.p; td.pt = x.t.pt; td.ptsum = x.t.ptsum;
				replay.feed( td );
			}
			if( best->wasLive && !replay.over ) replay.failed = replay.over = true;
			if( replay.failed != ( best->h.failed != 0 ) || (int)replay.tokens.size() != best->h.nTok || replay.resultLen != best->h.resultLen )
			{
				logError( "beam search: the device's stop rules and the host's disagree on the winning hypothesis (failed %d / %d, tokens %d / %d, resultLen %d / %d)",
					(int)replay.failed, best->h.failed, (int)replay.tokens.size(), best->h.nTok, replay.resultLen, best->h.resultLen );
				return E_UNEXPECTED;
			}
			result.adopt( replay );
			return S_OK;
		}

		// The device context a run with these parameters works on (see runFullImpl)
		HRESULT ContextImpl::activeContext( const sFullParams& params, bool warn, wh_context*& active, int& beamWidth )
		{
			beamWidth = 0;
			if( params.strategy == eSamplingStrategy::BeamSearch && params.beam_search.beam_width >= 1 )
			{
				beamWidth = params.beam_search.beam_width;
				if( beamWidth > 8 )
				{
					if( warn ) logWarning( "runFull: beam_width %d is more than this build decodes in lock step; using 8", beamWidth );
					beamWidth = 8;
				}
				CHECK( beamContext( beamWidth ) );
			}
			active = beamWidth >= 1 ? gpuBeam : gpu;
			return S_OK;
		}

		// whisper_lang_auto_detect (Whisper/source/whisper.cpp:2428-2495) on the window at `seek` of the context's spectrogram source: the encoder with the
		// model's full audio context, [sot] at position 0 and the language tokens' probabilities on the device (wh_lang_detect), the reference's second
		// softmax over them on the host (finishLanguageProbs). Like the reference, only the languages of the table take part (a vocabulary of the large-v3
		// shape has one token more). Leaves the window encoded and ready to be decoded.
		HRESULT ContextImpl::detectOnWindow( wh_context* ctx, int seek, std::vector<float>* probs, int& langId )
		{
			const int nDev = wh_model_lang_count( model->gpu );
			const int n = std::min( nDev, (int)languageList().length );
			if( n <= 0 ) return E_INVALIDARG;
			audioCtx = 0;
			CHECK_WH( wh_context_set_audio_ctx( ctx, 0 ) );
			const auto t = Clock::now();
			CHECK( encodeWindow( ctx, seek ) );
			msEncode += msSince( t );
			nEncode++;
			std::vector<float> p( (size_t)nDev );
			int32_t best = 0;
			CHECK_WH( wh_lang_detect( ctx, 1, p.data(), &best ) );
			std::vector<float> lp( (size_t)n );
			langId = finishLanguageProbs( p.data(), n, lp.data() );
			if( langId < 0 ) return E_UNEXPECTED;
			// a vocabulary with more language tokens than the table has languages (the large-v3 shape's 100th): the device's winner may be one of them
			if( best >= n )
				logWarning( "language detection: the most probable language token (id %d, p = %f) is not in the table of %d languages; using %s", (int)best,
					p[ (size_t)best ], n, languageCode( langId ).c_str() );
			detectedLang = langId;
			detectedP = lp[ (size_t)langId ];
			if( probs ) probs->swap( lp );
			return S_OK;
		}

		// The "auto" branch of whisper_full (whisper.cpp:2788-2801): detection on the window at FRAME 0 whatever offset_ms is, the winner replaces the
		// language, the reference's log line. Nothing is detected where the run would not decode anything anyway: an .en model (the language is not read),
		// less than a second of audio (S_FALSE), parameters StreamRun::begin rejects.
		HRESULT ContextImpl::resolveLanguage( sFullParams& params, bool& firstWindowEncoded )
		{
			firstWindowEncoded = false;
			detectedLang = -1;
			detectedP = 0;
			if( !model->vocab.isMultilingual() || !isLanguageAuto( params.language ) ) return S_OK;
			const int seekStart = params.offset_ms / 10;
			if( languageDetectionMoot( params, mel.length, model->hp ) )
			{
				params.language = makeLanguageKey( "en" );	   // never read: StreamRun::begin returns before the prompt is built
				return S_OK;
			}
			if( mel.length <= 0 )
			{
				logError( "runFull: failed to auto-detect language: no audio at the start of the buffer" );
				return E_INVALIDARG;
			}
			wh_context* active = nullptr;
			int beamWidth = 0;
			CHECK( activeContext( params, false, active, beamWidth ) );
			int langId = -1;
			CHECK( detectOnWindow( active, 0, nullptr, langId ) );
			const std::string code = languageCode( langId );
			params.language = makeLanguageKey( code.c_str() );
			logInfo( "whisper_full: auto-detected language: %s (p = %f)", code.c_str(), detectedP );
			firstWindowEncoded = seekStart == 0 && params.audio_ctx == 0;
			// a streamed spectrogram remembers where its last window ended (MelSource::lastBufferEnd): a window that is encoded again starts from a clean state
			if( !firstWindowEncoded ) mel.lastBufferEnd = -1;
			return S_OK;
		}

		// whisper_lang_auto_detect as an entry point of its own: the spectrogram of the whole buffer (runFull's), the window at offsetMs / 10
		HRESULT ContextImpl::detectLanguage( const float* pcm, uint32_t nSamples, int offsetMs, float* probs, uint32_t probsCap, int& langId )
		{
			langId = -1;
			detectedLang = -1;
			detectedP = 0;
			if( !model->vocab.isMultilingual() )
			{
				logError( "detectLanguage: the model is not multilingual" );
				return E_INVALIDARG;
			}
			const int seek = offsetMs / 10;
			const int64_t melLen = nSamples / 160;
			if( offsetMs < 0 )
			{
				logError( "whisper_lang_auto_detect: offset %dms is before the start of the audio", offsetMs );
				return E_INVALIDARG;
			}
			if( seek >= melLen )
			{
				logError( "whisper_lang_auto_detect: offset %dms is past the end of the audio (%dms)", offsetMs, (int)melLen * 10 );
				return E_INVALIDARG;
			}
			mel = MelSource{};
			mel.length = melLen;
			CHECK( ensureBuffer( pcmDev, pcmCapacity, (int64_t)nSamples * 4 ) );
			CHECK( ensureBuffer( melDev, melCapacity, melLen * model->hp.n_mels * 4 ) );
			CHECK_WH( wh_buffer_upload( gpu, pcmDev, pcm, (int64_t)nSamples * 4 ) );
			int64_t got = 0;
			CHECK_WH( wh_mel_spectrogram( gpu, (const float*)pcmDev, nSamples, (float*)melDev, &got ) );
			std::vector<float> lp;
			CHECK( detectOnWindow( gpu, seek, &lp, langId ) );
			if( probs ) memcpy( probs, lp.data(), sizeof( float ) * std::min( (size_t)probsCap, lp.size() ) );
			return S_OK;
		}

		HRESULT ContextImpl::runFullImpl( const sFullParams& paramsIn, const sProgressSink& progress )
		{
			// the stream's rules (seek range, prompt carry-over, stop rules, segments, callbacks) live in hostLoop.h, shared with the
			// lock-step scheduler of runFullBatch; here: the device work of ONE stream, window after window
			const Vocabulary& vocab = model->vocab;
			const wh_hparams& hp = model->hp;
			// language "auto": resolved HERE, before the stream's rules see the parameters (hostLoop.h knows languages of the table only)
			sFullParams params = paramsIn;
			bool firstWindowEncoded = false;
			CHECK( resolveLanguage( params, firstWindowEncoded ) );
			// AlignTokens: one stream, decoded greedily (beam search is a follow-up: the compute entry point is batched for it already)
			if( params.flag( eFullParamsFlags::AlignTokens ) && params.strategy == eSamplingStrategy::BeamSearch && params.beam_search.beam_width >= 1 )
			{
				logError( "runFull: eFullParamsFlags::AlignTokens is not available with eSamplingStrategy::BeamSearch" );
				return E_NOTIMPL;
			}
			// decoding fallback: one stream, the Greedy strategy (the batch runner and beam search are follow-ups)
			windowStats.clear();
			if( fallbackOn && params.strategy == eSamplingStrategy::BeamSearch && params.beam_search.beam_width >= 1 )
			{
				logError( "runFull: decoding fallback (setDecodingFallback) is not available with eSamplingStrategy::BeamSearch" );
				return E_NOTIMPL;
			}
			// timestamp rules: the device-side loop only (the records would have to follow the beam's parent reorder: a follow-up)
			if( timestampRulesOn && params.strategy == eSamplingStrategy::BeamSearch && params.beam_search.beam_width >= 1 )
			{
				logError( "runFull: the timestamp rules (setTimestampRules) are not available with eSamplingStrategy::BeamSearch" );
				return E_NOTIMPL;
			}
			// boosted phrases: the device-side loop only (the per-sequence states would have to follow the beam's parent reorder: a follow-up)
			if( boostOn && params.strategy == eSamplingStrategy::BeamSearch && params.beam_search.beam_width >= 1 )
			{
				logError( "runFull: boosted phrases (setBoostedPhrases) are not available with eSamplingStrategy::BeamSearch" );
				return E_NOTIMPL;
			}
			// no-repeat n-grams: the device-side loop only (the per-sequence histories would have to follow the beam's parent reorder)
			if( noRepeatN && params.strategy == eSamplingStrategy::BeamSearch && params.beam_search.beam_width >= 1 )
			{
				logError( "runFull: no-repeat n-grams (setNoRepeatNgram) are not available with eSamplingStrategy::BeamSearch" );
				return E_NOTIMPL;
			}
			StreamRun run( params, vocab, hp, this, progress, resultAll, promptPast, &stamper );
			// the run's audio is current until this function returns; the stereo PCM is the caller's and is not referred to afterwards
			struct CurrentRun
			{
				ContextImpl& c;
				explicit CurrentRun( ContextImpl& ctx ) : c( ctx ) { c.runCurrent = true; c.speakers.clear(); }
				~CurrentRun() { c.runCurrent = false; c.stereoPcm = nullptr; c.stereoFrames = 0; }
			} current( *this );
			const HRESULT hrBegin = run.begin( mel.length );
			if( hrBegin != S_OK ) return hrBegin;
			// eSamplingStrategy::BeamSearch (declared by the reference, implemented only here: sFullParams.h:10-13): beam_width hypotheses per
			// window through decodeWindowBeam (width 1 included: there it must reproduce the greedy loop token for token). The Greedy strategy
			// takes the device-side greedy loop.
			int beamWidth = 0;
			// the ONE device context this run works on: the window x hypotheses context of a beam search, else the stream's own
			wh_context* active = nullptr;
			CHECK( activeContext( params, true, active, beamWidth ) );
			// overwrite audio_ctx (ContextImpl.cpp:488-489): encoder positions and cross-attention keys of every window of this run
			audioCtx = params.audio_ctx;
			CHECK_WH( wh_context_set_audio_ctx( active, audioCtx ) );
			// AlignTokens: a finished window's text against its cross-attention caches, which are still the window's when StreamRun::finishWindow asks
			struct DeviceAligner : iTokenAligner
			{
				wh_context* ctx;
				const Vocabulary& vocab;
				int64_t melLen;
				int keysMax;
				DeviceAligner( wh_context* c, const Vocabulary& v, int64_t len, int keys ) : ctx( c ), vocab( v ), melLen( len ), keysMax( keys ) {}
				HRESULT alignWindow( int seek, int seekEnd, const std::vector<int>& sotSequence, const std::vector<int>& text, std::vector<int>& frames ) override
				{
					std::vector<int32_t> tokens( sotSequence.begin(), sotSequence.end() );
					tokens.push_back( vocab.token_not );
					tokens.insert( tokens.end(), text.begin(), text.end() );
					tokens.push_back( vocab.token_eot );
					const int32_t len = (int32_t)tokens.size();
					const int64_t audioEnd = std::min<int64_t>( seekEnd, melLen );
					const int32_t nKeys = (int32_t)std::max<int64_t>( 1, std::min<int64_t>( keysMax, ( audioEnd - seek ) / 2 ) );
					std::vector<int32_t> all( tokens.size() );
					CHECK_WH( wh_align_tokens( ctx, 1, tokens.data(), &len, &nKeys, len, all.data() ) );
					frames.assign( all.begin(), all.begin() + (ptrdiff_t)text.size() + 1 );
					return S_OK;
				}
			} aligner( active, vocab, mel.length, audioCtx > 0 ? audioCtx : hp.n_audio_ctx );
			if( params.flag( eFullParamsFlags::AlignTokens ) ) run.setAligner( &aligner );
			// speech only: the spectrogram is that of the packed speech; what the run reports is on the recording's clock
			if( !runMap.empty() ) run.setTimeMap( &runMap );
			// decoding fallback: whatever path leaves this function, the context is back at the greedy sampler and gathers nothing
			struct SamplingGuard
			{
				wh_context* const ctx;
				~SamplingGuard()
				{
					if( !ctx ) return;
					wh_context_set_sampling( ctx, 0.0f, 0, 0 );
					wh_context_set_no_speech( ctx, 0 );
				}
			} samplingGuard{ fallbackOn ? active : nullptr };
			std::vector<int> prompt;
			// one greedy-loop pass over the window the encoder just filled: at the context's temperature when it has one
			auto decodeAttempt = [ & ]( WindowDecoder& dec, WindowScan& scan ) -> HRESULT
			{
				for( bool first = true; !scan.over; first = false )
				{
					TokenData token;
					if( first )
						CHECK( dec.start( prompt, token ) );
					else
						CHECK( dec.next( token ) );
					scan.feed( token );
				}
				return S_OK;
			};
			while( true )
			{
				const HRESULT hrNext = run.nextWindow( prompt );
				if( FAILED( hrNext ) ) return hrNext;
				if( hrNext != S_OK ) break;
				{
					// enqueued without a host sync: the decoder's launches line up behind the encoder's on the context's stream.
					// With WHISPER_PROFILE=1 the two are separated so that the "Encode" block means what it means in the reference.
					const auto t = Clock::now();
					// the window language detection encoded (frame 0, the full audio context) is this run's first window: not encoded twice
					const bool encoded = firstWindowEncoded && run.seek == 0;
					firstWindowEncoded = false;
					if( !encoded )
					{
						CHECK( encodeWindow( active, run.seek ) );
						if( gpuProfile ) CHECK_WH( wh_context_synchronize( active ) );	   // the context the encoder was queued on ("Encode" measures the encoder, not its enqueue)
						msEncode += msSince( t );
						nEncode++;
					}
				}
				const auto tDec = Clock::now();
				WindowDecoder dec( active, hp.n_text_ctx );
				WindowScan scan( run.fullParams(), vocab, run.seek, run.seekEnd(), run.maxTokens() );
				if( beamWidth >= 1 )
					CHECK( g_beamRankingOnHost ? decodeWindowBeam( prompt, beamWidth, scan, dec.steps ) : decodeWindowBeamDevice( prompt, beamWidth, scan, dec.steps ) );
				else if( !fallbackOn )
					CHECK( decodeAttempt( dec, scan ) );
				else
				{
					// the plan of decodeFallback.h around the greedy loop: the encoder output and the cross-attention caches stay the window's, a further
					// attempt is one more decode from position 0. The no-speech probability is the greedy attempt's (temperature 0: the model's own
					// distribution, as openai-whisper takes it); later attempts do not gather it again.
					fallback::FallbackPlan plan( fallbackParams, run.seek );
					sWindowStats ws = {};
					ws.seek = run.seek;
					int steps = 0;
					while( true )
					{
						const float temperature = plan.temperature();
						CHECK_WH( wh_context_set_sampling( active, temperature, plan.seed(), plan.nonce() ) );
						CHECK_WH( wh_context_set_no_speech( active, plan.attemptIndex() == 0 ? 1 : 0 ) );
						WindowDecoder attemptDec( active, hp.n_text_ctx );
						WindowScan attemptScan( run.fullParams(), vocab, run.seek, run.seekEnd(), run.maxTokens() );
						CHECK( decodeAttempt( attemptDec, attemptScan ) );
						if( plan.attemptIndex() == 0 ) CHECK_WH( wh_decode_window_no_speech( active, &ws.noSpeech ) );
						steps += attemptDec.steps;
						dec.msFetch += attemptDec.msFetch;
						dec.msEnqueue += attemptDec.msEnqueue;
						fallback::Attempt a;
						a.scanFailed = attemptScan.failed;
						a.resultLen = std::min( attemptScan.resultLen, (int)attemptScan.tokens.size() );
						a.scores = fallback::score( attemptScan.tokens.data(), a.resultLen );
						a.noSpeech = ws.noSpeech;
						ws.attempts = plan.attempts();
						ws.temperature = temperature;
						ws.avgLogprob = a.scores.avgLogprob;
						ws.entropy = a.scores.entropy;
						const fallback::eVerdict verdict = plan.judge( a );
						if( verdict == fallback::eVerdict::Retry ) continue;
						scan.adopt( attemptScan );
						if( verdict == fallback::eVerdict::Skip )
						{
							// silence: no segments, nothing for the next window's prompt, the stream moves on by the scan's seekDelta
							scan.tokens.clear();
							scan.resultLen = 0;
							ws.skipped = 1;
						}
						break;
					}
					dec.steps = steps;
					windowStats.push_back( ws );
				}
				msDecode += msSince( tDec );
				if( getenv( "WHISPER_HOSTPROF" ) )
					fprintf( stderr, "[hostprof] window at %d: decode %.2f ms for %d tokens, of which waiting for samples %.2f ms, enqueueing steps %.2f ms\n", run.seek,
						msSince( tDec ), dec.steps, dec.msFetch, dec.msEnqueue );
				nDecodeSteps += dec.steps;	   // tokens the loop consumed (the reference counts one DecodeStep per token)
				nDecodeWindows++;
				const HRESULT hrWindow = run.finishWindow( scan );
				appendSpeakers( resultAll, mediaTimeOffset, stereoPcm, stereoFrames, speakers );
				CHECK( hrWindow );
			}
			return run.end();
		}

		HRESULT ContextImpl::fillResults( eResultFlags flags, ResultData& res ) const
		{
			// a segment whose new_segment callback is running has not been through runFullImpl's own call yet
			if( runCurrent ) appendSpeakers( resultAll, mediaTimeOffset, stereoPcm, stereoFrames, speakers );
			res.speakers.assign( speakers.begin(), speakers.begin() + std::min( speakers.size(), resultAll.size() ) );
			return fillResultData( resultAll, model->vocab, mediaTimeOffset, flags, res );
		}

		HRESULT ContextImpl::getResults( eResultFlags flags, iTranscribeResult** pp ) const
		{
			if( !pp ) return E_POINTER;
			if( flags & eResultFlags::NewObject )
			{
				TranscribeResult* r = new TranscribeResult();
				const HRESULT hr = fillResults( flags, *r );
				if( FAILED( hr ) ) { r->Release(); return hr; }
				*pp = r;
				return S_OK;
			}
			CHECK( fillResults( flags, results ) );
			*pp = &results;
			return S_OK;
		}

		// ---- iModel -----------------------------------------------------------------------------------------------
		class ModelImpl : public ComObject<iModel>, public iModelInternals
		{
			std::shared_ptr<LoadedModel> model;
		public:
			explicit ModelImpl( const std::shared_ptr<LoadedModel>& m ) : model( m ) {}
			HRESULT QueryInterface( const ComLight::GUID& riid, void** ppv ) override
			{
				if( ppv && riid == iModelInternals::iid() )
				{
					*ppv = static_cast<iModelInternals*>( this );
					ComObject<iModel>::AddRef();
					return S_OK;
				}
				return ComObject<iModel>::QueryInterface( riid, ppv );
			}
			uint32_t AddRef() override { return ComObject<iModel>::AddRef(); }
			uint32_t Release() override { return ComObject<iModel>::Release(); }
			const std::shared_ptr<LoadedModel>& loaded() const override { return model; }
			HRESULT createContext( iContext** pp ) override { return createContextImpl( model, this, pp ); }
			HRESULT tokenize( const char* text, pfnDecodedTokens pfn, void* pv ) override
			{
				if( !pfn ) return E_POINTER;
				std::vector<int> toks;
				CHECK( model->vocab.tokenize( text, toks ) );
				pfn( toks.empty() ? nullptr : toks.data(), (int)toks.size(), pv );
				return S_OK;
			}
			HRESULT isMultilingual() override { return model->vocab.isMultilingual() ? S_OK : S_FALSE; }
			HRESULT getSpecialTokens( SpecialTokens& r ) override
			{
				const Vocabulary& v = model->vocab;
				r.TranscriptionEnd = v.token_eot; r.TranscriptionStart = v.token_sot; r.PreviousWord = v.token_prev;
				r.SentenceStart = v.token_solm; r.Not = v.token_not; r.TranscriptionBegin = v.token_beg;
				r.TaskTranslate = v.token_translate; r.TaskTranscribe = v.token_transcribe;
				return S_OK;
			}
			const char* stringFromToken( whisper_token token ) override { return model->vocab.string( token ); }
			// Weights are immutable and shared (WhisperModel.h:28-30): a clone is another handle on the same arena, so that
			// a second context can run from another host thread (ModelImpl.cpp:40-60 needs OpenSharedResource for this).
			HRESULT clone( iModel** rdi ) override { return createModelImpl( model, rdi ); }
		};

		// ---- iMediaFoundation stand-in: WAV (plain PCM of any rate, wavFormat.h) ---------------------------------------
		class WavLoader : public ComObject<iMediaFoundation>
		{
		public:
			HRESULT loadAudioFile( LPCTSTR path, bool stereo, iAudioBuffer** pp ) const override;
			HRESULT openAudioFile( LPCTSTR path, bool stereo, iAudioReader** pp ) override;
			HRESULT loadAudioFileData( const void* data, uint64_t size, bool stereo, iAudioReader** pp ) override;
			HRESULT listCaptureDevices( pfnFoundCaptureDevices, void* ) override { return E_NOTIMPL; }
			HRESULT openCaptureDevice( LPCTSTR, const sCaptureParams&, iAudioCapture** ) override { return E_NOTIMPL; }
		};

		// RIFF/WAVE (wavFormat.h: PCM of 8 .. 32 bits or float32, 1 .. 8 channels, 1000 .. 384000 Hz) -> 16 kHz mono (and interleaved stereo when asked for: the
		// first two channels; a mono file has no stereo data, like the reference's buffer of a mono source, Whisper/MF/loadAudioFile.cpp:61-63). The mean of the
		// channels is their FP32 sum in channel order times 1.0f / C. A 16 kHz file is converted here;
		// any other rate goes to the GPU in the file's own format (wh_resample_host on the calling thread's current device: conversion, downmix and the filter).
		static HRESULT decodeWav( const char* bytes, size_t size, const std::string& what, bool wantStereo, std::vector<float>& mono, std::vector<float>& st )
		{
			wav::Info info;
			std::string error;
			if( !wav::parse( bytes, size, info, error ) )
			{
				logError( "'%s': %s", what.c_str(), error.c_str() );
				return E_INVALIDARG;
			}
			if( info.channels < 2 ) wantStereo = false;
			const uint8_t* const pcm = (const uint8_t*)bytes + info.firstByte;
			const int channels = info.channels, right = channels >= 2 ? 1 : 0;
			st.clear();
			if( info.rate == 16000 )
			{
				const size_t frames = info.frames, step = (size_t)wav::bytesPerSample( info.format );
				mono.resize( frames );
				if( wantStereo ) st.resize( frames * 2 );
				const float inv = 1.0f / (float)channels;
				for( size_t i = 0; i < frames; i++ )
				{
					const uint8_t* const f = pcm + i * channels * step;
					const float l = wav::sample( f, info.format );
					float sum = l;
					for( int c = 1; c < channels; c++ ) sum += wav::sample( f + c * step, info.format );
					mono[ i ] = channels == 1 ? l : sum * inv;
					if( wantStereo ) { st[ 2 * i ] = l; st[ 2 * i + 1 ] = wav::sample( f + right * step, info.format ); }
				}
				return S_OK;
			}
			int64_t nOut = 0;
			if( 0 != wh_resample_out_len( info.rate, (int64_t)info.frames, &nOut ) ) return E_INVALIDARG;
			mono.resize( (size_t)nOut );
			if( wantStereo ) st.resize( (size_t)nOut * 2 );
			if( nOut == 0 ) return S_OK;
			// one upload: the mono mix and, when asked for, the two stereo channels interleaved
			const int32_t list[ 3 ] = { -1, 0, right };
			float* const dsts[ 3 ] = { mono.data(), st.data(), st.data() + 1 };
			const int64_t strides[ 3 ] = { 1, 2, 2 };
			CHECK_WH( wh_resample_host_multi( pcm, info.format, channels, list, wantStereo ? 3 : 1, info.rate, (int64_t)info.frames, dsts, strides, nOut ) );
			return S_OK;
		}
		static HRESULT readWavFile( LPCTSTR path, bool stereo, std::vector<float>& mono, std::vector<float>& st )
		{
			const std::string p = path;	  // LPCTSTR is UTF-8 off Windows (ComLightLib/comLightCommon.h:8)
			std::ifstream f( p, std::ios::binary );
			if( !f ) { logError( "failed to open audio file '%s'", p.c_str() ); return (HRESULT)0x80070002; }
			std::vector<char> data( ( std::istreambuf_iterator<char>( f ) ), std::istreambuf_iterator<char>() );
			return decodeWav( data.data(), data.size(), p, stereo, mono, st );
		}

		HRESULT WavLoader::loadAudioFile( LPCTSTR path, bool stereo, iAudioBuffer** pp ) const
		{
			if( !pp || !path ) return E_POINTER;
			std::vector<float> mono, st;
			CHECK( readWavFile( path, stereo, mono, st ) );
			return createAudioBuffer( std::move( mono ), std::move( st ), pp );
		}
		HRESULT WavLoader::openAudioFile( LPCTSTR path, bool stereo, iAudioReader** pp )
		{
			if( !pp || !path ) return E_POINTER;
			std::vector<float> mono, st;
			CHECK( readWavFile( path, stereo, mono, st ) );
			*pp = new WavReader( std::move( mono ), std::move( st ), stereo );
			return S_OK;
		}
		HRESULT WavLoader::loadAudioFileData( const void* data, uint64_t size, bool stereo, iAudioReader** pp )
		{
			if( !pp || !data ) return E_POINTER;
			std::vector<float> mono, st;
			CHECK( decodeWav( (const char*)data, (size_t)size, "<memory>", stereo, mono, st ) );
			*pp = new WavReader( std::move( mono ), std::move( st ), stereo );
			return S_OK;
		}
	}	// namespace

	// whisper_full_default_params as the reference restates it (ContextImpl.misc.cpp:61-93): what iContext::fullDefaultParams answers, and it reads nothing of a context
	HRESULT defaultFullParams( eSamplingStrategy strategy, sFullParams* rdi )
	{
		if( !rdi ) return E_POINTER;
		memset( rdi, 0, sizeof( sFullParams ) );
		rdi->strategy = strategy;
		rdi->cpuThreads = 4;
		rdi->n_max_text_ctx = 16384;
		rdi->flags = eFullParamsFlags::PrintProgress | eFullParamsFlags::PrintTimestamps;
		rdi->thold_pt = rdi->thold_ptsum = 0.01f;
		rdi->language = makeLanguageKey( "en" );
		switch( strategy )
		{
		case eSamplingStrategy::Greedy:
			rdi->beam_search.n_past = rdi->beam_search.beam_width = rdi->beam_search.n_best = -1;
			return S_OK;
		case eSamplingStrategy::BeamSearch:
			rdi->greedy.n_past = -1;
			rdi->beam_search.beam_width = 10;
			rdi->beam_search.n_best = 5;
			return S_OK;
		}
		logError( "Unknown sampling strategy %i", (int)strategy );
		return E_INVALIDARG;
	}
	void setBeamRankingOnHost( bool onHost ) { g_beamRankingOnHost = onHost; }

	// flatApi.cpp reaches the methods that are not part of iContext's vtable (every iContext of this library is a ContextImpl)
	HRESULT contextDetectLanguage( void* ctx, const float* pcm, uint32_t nSamples, int offsetMs, float* probs, uint32_t probsCap, int& langId )
	{
		return static_cast<ContextImpl*>( (iContext*)ctx )->detectLanguage( pcm, nSamples, offsetMs, probs, probsCap, langId );
	}
	int contextDetectedLanguage( void* ctx, float& p )
	{
		return static_cast<ContextImpl*>( (iContext*)ctx )->lastDetectedLanguage( p );
	}
	HRESULT contextSetDeviceFlags( void* ctx, uint32_t flags, int parityThreads )
	{
		return static_cast<ContextImpl*>( (iContext*)ctx )->setDeviceFlags( flags, parityThreads );
	}
	HRESULT contextRunCapture( void* ctx, const sFullParams& params, const sCaptureCallbacks& callbacks, const iAudioCapture* reader, pfnCapturePiece pfnPiece, void* pvPiece )
	{
		return static_cast<ContextImpl*>( (iContext*)ctx )->runCapturePieces( params, callbacks, reader, pfnPiece, pvPiece );
	}
	// a reader over PCM that is decoded already (whisperc_run_streamed_stereo): what loadAudioFileData makes of a WAV image, with the caller's stereo PCM
	HRESULT createPcmReader( std::vector<float>&& mono, std::vector<float>&& stereo, iAudioReader** pp )
	{
		if( !pp ) return E_POINTER;
		const bool wantStereo = !stereo.empty();
		*pp = new WavReader( std::move( mono ), std::move( stereo ), wantStereo );
		return S_OK;
	}
	// capture.cpp's way to the device half of a capture at another rate than 16 kHz (captureRate.h): installed when the library is loaded
	static const CaptureRateTable g_captureRateEntries = { &wh_capture_create_rate, &wh_capture_flush, &wh_capture_skip };
	static const bool g_captureRateInstalled = ( g_captureRateTable = &g_captureRateEntries, true );
	// the lock-step scheduler's way to the device half of language detection (languageDetect.h): installed when the library is loaded
	static const bool g_detectorInstalled = ( g_batchLanguageDetector = &wh_lang_detect, true );
	// ... and to per-row sampling and the no-speech gather (batchSampling.h)
	static const BatchSamplingHooks g_samplingHooks = { &wh_context_set_sampling_rows, &wh_context_set_no_speech, &wh_decode_window_no_speech };
	static const bool g_samplingInstalled = ( g_batchSamplingHooks = &g_samplingHooks, true );
	// ... and to the logit filter of suppressed tokens (batchSuppress.h)
	static const bool g_suppressInstalled = ( g_batchSuppress = &wh_context_set_suppress, true );
	// ... and to the timestamp rules (batchTimestampRules.h)
	static const bool g_timestampRulesInstalled = ( g_batchTimestampRules = &wh_context_set_timestamp_rules, true );
	// ... and to the phrase filter (batchBoost.h)
	static const bool g_boostInstalled = ( g_batchBoost = &wh_context_set_boost, true );
	// ... and to the n-gram filter (batchNoRepeat.h)
	static const bool g_noRepeatInstalled = ( g_batchNoRepeat = &wh_context_set_no_repeat, true );
	// ... and to the scorer of given transcripts (scoreRequest.h)
	static const bool g_scorerInstalled = ( g_batchScorer = &wh_score_tokens, true );
	// ... and to the speech filter of a newly admitted stream (batchSpeech.h)
	static const bool g_speechPackerInstalled = ( g_batchSpeechPacker = &wh_context_speech_filter, true );

	HRESULT createContextImpl( const std::shared_ptr<LoadedModel>& model, iModel* owner, iContext** pp )
	{
		if( !pp ) return E_POINTER;
		ContextImpl* c = new ContextImpl( model, owner );
		const HRESULT hr = c->init();
		if( FAILED( hr ) ) { c->Release(); return hr; }
		*pp = c;
		return S_OK;
	}
	HRESULT setAlignmentHeads( iModel* model, const int32_t* layerHeadPairs, uint32_t count )
	{
		if( !model || ( count && !layerHeadPairs ) ) return E_POINTER;
		iModelInternals* in = nullptr;
		if( FAILED( model->QueryInterface( iModelInternals::iid(), (void**)&in ) ) || !in )
		{
			logError( "setAlignmentHeads: the model was not created by this library" );
			return E_INVALIDARG;
		}
		const int rc = wh_model_set_alignment_heads( in->loaded()->gpu, layerHeadPairs, (int)count );
		model->Release();	  // QueryInterface's reference
		CHECK_WH( rc );
		return S_OK;
	}
	// the options of a context: the public function on the ContextImpl behind `context` (optionRules::forward)
	static const char* const NOT_A_CONTEXT = "not a context of this library's createContext";
	HRESULT setDecodingFallback( iContext* context, const sDecodingFallback* params )
	{
		return optionRules::forward<ContextImpl>( context, "setDecodingFallback", NOT_A_CONTEXT, "a batch runner takes setBatchDecodingFallback",
			[ = ]( ContextImpl& c ) { return c.setFallback( params ); } );
	}
	HRESULT setSuppressedTokens( iContext* context, const int32_t* ids, uint32_t count )
	{
		return optionRules::forward<ContextImpl>( context, "setSuppressedTokens", NOT_A_CONTEXT, "a batch runner takes setBatchSuppressedTokens",
			[ = ]( ContextImpl& c ) { return c.setSuppressed( ids, count ); } );
	}
	HRESULT setTimestampRules( iContext* context, bool on )
	{
		return optionRules::forward<ContextImpl>( context, "setTimestampRules", NOT_A_CONTEXT, "a batch runner takes setBatchTimestampRules",
			[ = ]( ContextImpl& c ) { return c.setTimestampRulesMode( on ); } );
	}
	HRESULT setBoostedPhrases( iContext* context, const sBoostedPhrases* phrases )
	{
		return optionRules::forward<ContextImpl>( context, "setBoostedPhrases", NOT_A_CONTEXT, "a batch runner takes setBatchBoostedPhrases",
			[ = ]( ContextImpl& c ) { return c.setBoosted( phrases ); } );
	}
	HRESULT setNoRepeatNgram( iContext* context, int n )
	{
		return optionRules::forward<ContextImpl>( context, "setNoRepeatNgram", NOT_A_CONTEXT, "a batch runner takes setBatchNoRepeatNgram",
			[ = ]( ContextImpl& c ) { return c.setNoRepeat( n ); } );
	}
	HRESULT setSpeechFilter( iContext* context, const sSpeechFilter* params )
	{
		return optionRules::forward<ContextImpl>( context, "setSpeechFilter", NOT_A_CONTEXT, "a batch runner takes setBatchSpeechFilter",
			[ = ]( ContextImpl& c ) { return c.setSpeech( params ); } );
	}
	HRESULT getSpeechSpans( const iContext* context, sSpeechSpan* spans, uint32_t* count )
	{
		if( !context || !count ) return E_POINTER;
		const ContextImpl* const c = dynamic_cast<const ContextImpl*>( context );
		if( !c ) return E_INVALIDARG;
		const std::vector<speechRules::Span>& all = c->lastSpeechSpans();
		const uint32_t cap = *count;
		*count = (uint32_t)all.size();
		if( !spans ) return S_OK;
		if( cap < all.size() ) return E_BOUNDS;
		for( size_t i = 0; i < all.size(); i++ ) spans[ i ] = sSpeechSpan{ all[ i ].a, all[ i ].b };
		return S_OK;
	}
	HRESULT contextScoreClip( iContext* context, const float* pcm, int64_t nSamples, const int32_t* tokens, int32_t len, int32_t firstScored, wh_token_score* recs, int32_t* frames )
	{
		if( !pcm || !tokens || !recs ) return E_POINTER;
		return optionRules::forward<ContextImpl>( context, "scoreTokens", NOT_A_CONTEXT, "a batch runner takes scoreBatch",
			[ = ]( ContextImpl& c ) { return c.scoreClip( pcm, nSamples, tokens, len, firstScored, recs, frames ); } );
	}
	HRESULT getWindowStats( const iContext* context, sWindowStats* stats, uint32_t* count )
	{
		if( !context || !count ) return E_POINTER;
		const ContextImpl* const c = dynamic_cast<const ContextImpl*>( context );
		if( !c ) return E_INVALIDARG;
		const std::vector<sWindowStats>& all = c->lastWindowStats();
		const uint32_t cap = *count;
		*count = (uint32_t)all.size();
		if( !stats ) return S_OK;
		if( cap < all.size() ) return E_BOUNDS;
		std::copy( all.begin(), all.end(), stats );
		return S_OK;
	}
	HRESULT createModelImpl( const std::shared_ptr<LoadedModel>& model, iModel** pp )
	{
		if( !pp ) return E_POINTER;
		*pp = new ModelImpl( model );
		return S_OK;
	}
	HRESULT createAudioBuffer( std::vector<float>&& mono, std::vector<float>&& stereo, iAudioBuffer** pp )
	{
		if( !pp ) return E_POINTER;
		AudioBuffer* b = new AudioBuffer();
		b->mono = std::move( mono );
		b->stereo = std::move( stereo );
		*pp = b;
		return S_OK;
	}

	// ---- exports ----------------------------------------------------------------------------------------------------
	static HRESULT loadModelImpl( const wchar_t* path, const sModelSetup& setup, const sLoadModelCallbacks* callbacks, wh_comm* comm, int root, iModel** pp );
	HRESULT loadModel( const wchar_t* path, const sModelSetup& setup, const sLoadModelCallbacks* callbacks, iModel** pp )
	{
		return loadModelImpl( path, setup, callbacks, nullptr, 0, pp );
	}
	// One process per GPU (extension; the reference has one GPU per model, ModelImpl.cpp:40-60): every rank calls this with its
	// own sModelSetup.adapter and the communicator of include/whisper_hip.h; rank `root` reads the file, the others receive the
	// weights over xGMI (RCCL broadcast) and read only the file's header.
	HRESULT loadModelShared( const wchar_t* path, const sModelSetup& setup, const sLoadModelCallbacks* callbacks, void* whComm, int root, iModel** pp )
	{
		if( !whComm ) return E_POINTER;
		return loadModelImpl( path, setup, callbacks, (wh_comm*)whComm, root, pp );
	}
	static HRESULT loadModelImpl( const wchar_t* path, const sModelSetup& setup, const sLoadModelCallbacks* callbacks, wh_comm* comm, int root, iModel** pp )
	{
		if( !path || !pp ) return E_POINTER;
		if( setup.impl != eModelImplementation::GPU )
		{
			// Hybrid is compiled out in the reference as well (stdafx.h:34); Reference is the vendored CPU model, which this
			// repository keeps as its test oracle (oracle/) and never links into the product.
			logError( "loadModel: only eModelImplementation::GPU is available in this build" );
			return E_NOTIMPL;
		}
		int device = 0;
		if( setup.adapter && *setup.adapter )
		{
			// What listGPUs hands out is "<index>: <name>"; the reference matches the adapter by its listed name
			// (Whisper/D3D/createDevice.cpp). Accepted: the full listed string, the name alone, or the bare index ("2" / "2:").
			const std::string a = utf8( setup.adapter );
			const int nDev = wh_device_count();
			device = -1;
			size_t digits = 0;
			while( digits < a.size() && isdigit( (unsigned char)a[ digits ] ) ) digits++;
			if( digits > 0 && ( digits == a.size() || ( digits + 1 == a.size() && a[ digits ] == ':' ) ) )
				device = atoi( a.c_str() );
			else
				for( int i = 0; i < nDev && device < 0; i++ )
				{
					char name[ 256 ];
					if( 0 != wh_device_info( i, name, sizeof( name ), nullptr, nullptr ) ) continue;
					if( a == std::to_string( i ) + ": " + name || a == name ) device = i;
				}
			if( device < 0 || device >= nDev )
			{
				logError( "loadModel: adapter '%s' not found (see listGPUs)", a.c_str() );
				return E_INVALIDARG;
			}
		}
		std::shared_ptr<LoadedModel> lm;
		CHECK( loadGgmlFile( utf8( path ), device, callbacks, lm, comm, root ) );
		return createModelImpl( lm, pp );
	}

	HRESULT initMediaFoundation( iMediaFoundation** pp )
	{
		if( !pp ) return E_POINTER;
		*pp = new WavLoader();
		return S_OK;
	}
}
