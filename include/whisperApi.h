// whisperApi.h -- public C++ API of libWhisper.so: the COM-style surface of Const-me/Whisper's Whisper.dll on Linux.
//
// A caller written against the reference (Examples/main/main.cpp:174-330, or the C# interop in WhisperNet/Internal)
// binds to these names, vtable layouts and POD structures unchanged:
//   exports      Whisper/whisper.def:1-8 ; declarations Whisper/API/iContext.cl.h:62-70, iMediaFoundation.cl.h:47
//   interfaces   iModel / iContext (Whisper/API/iContext.cl.h:23-60), iTranscribeResult (iTranscribeResult.cl.h:7-15),
//                iAudioBuffer / iAudioReader / iAudioCapture / iMediaFoundation (iMediaFoundation.cl.h:8-45)
//   structures   sFullParams (sFullParams.h:45-108), sModelSetup (sModelSetup.h), sSegment / sToken (TranscribeStructs.h)
// Binary contract = ComLight's (ComLightLib/comLightCommon.h, unknwn.h): every interface starts with
// QueryInterface / AddRef / Release, then its methods in declaration order; objects are intrusively ref-counted and
// factories return them with one reference through a T** out-parameter; HRESULT everywhere, S_FALSE = benign "no".
// This header is written from that contract, not copied: types that the Linux build cannot honour (Media Foundation
// readers, capture devices) are kept so vtable slots line up, and return E_NOTIMPL.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef WHISPER_EXPORT
#define WHISPER_EXPORT __attribute__( ( visibility( "default" ) ) )
#endif

typedef int32_t HRESULT;
#ifndef S_OK
#define S_OK ( (HRESULT)0 )
#define S_FALSE ( (HRESULT)1 )
#define E_NOTIMPL ( (HRESULT)0x80004001 )
#define E_NOINTERFACE ( (HRESULT)0x80004002 )
#define E_POINTER ( (HRESULT)0x80004003 )
#define E_FAIL ( (HRESULT)0x80004005 )
#define E_UNEXPECTED ( (HRESULT)0x8000FFFF )
#define E_OUTOFMEMORY ( (HRESULT)0x8007000E )
#define E_INVALIDARG ( (HRESULT)0x80070057 )
#define E_BOUNDS ( (HRESULT)0x8000000B )
#define OLE_E_BLANK ( (HRESULT)0x80040007 )	   // iContext::detectSpeaker outside a run
#define SUCCEEDED( hr ) ( ( (HRESULT)( hr ) ) >= 0 )
#define FAILED( hr ) ( ( (HRESULT)( hr ) ) < 0 )
#endif

struct IMFSourceReader;	   // Windows-only type, never defined here
// The reference's path type for media files: TCHAR* = UTF-16 on Windows, `using LPCTSTR = const char*` (UTF-8) everywhere
// else (ComLightLib/comLightCommon.h:5-9). A caller compiled from the reference's own headers on Linux passes const char*.
#ifndef _MSC_VER
using LPCTSTR = const char*;
#endif

namespace ComLight
{
	struct GUID
	{
		uint32_t Data1;
		uint16_t Data2, Data3;
		uint8_t Data4[ 8 ];
		bool operator==( const GUID& o ) const { return 0 == memcmp( this, &o, sizeof( GUID ) ); }
	};

	// {00000000-0000-0000-C000-000000000046}
	struct IUnknown
	{
		virtual HRESULT QueryInterface( const GUID& riid, void** ppvObject ) = 0;
		virtual uint32_t AddRef() = 0;
		virtual uint32_t Release() = 0;
	};
	constexpr GUID IID_IUnknown = { 0, 0, 0, { 0xC0, 0, 0, 0, 0, 0, 0, 0x46 } };

	// minimal smart pointer for callers and tests
	template<class I>
	class CComPtr
	{
		I* p = nullptr;
	public:
		CComPtr() = default;
		CComPtr( const CComPtr& o ) : p( o.p ) { if( p ) p->AddRef(); }
		~CComPtr() { release(); }
		CComPtr& operator=( const CComPtr& o ) { if( o.p ) o.p->AddRef(); release(); p = o.p; return *this; }
		void release() { if( p ) { p->Release(); p = nullptr; } }
		I** operator&() { release(); return &p; }
		I* operator->() const { return p; }
		operator I*() const { return p; }
		I* detach() { I* r = p; p = nullptr; return r; }
	};
}

namespace Whisper
{
	using whisper_token = int;
	struct iContext;
	struct iModel;

	// ---- plain-old-data ----------------------------------------------------------------------------------------
	enum struct eModelImplementation : uint32_t
	{
		GPU = 1,		// here: the MI355X HIP path
		Hybrid = 2,		// not built (disabled in the reference too, Whisper/stdafx.h:34)
		Reference = 3,	// the vendored CPU model; not part of the product library (it is the test oracle)
	};
	enum struct eGpuModelFlags : uint32_t
	{
		Wave32 = 1, Wave64 = 2, NoReshapedMatMul = 4, UseReshapedMatMul = 8, Cloneable = 0x10,
	};
	struct sModelSetup
	{
		eModelImplementation impl = eModelImplementation::GPU;
		uint32_t flags = 0;
		const wchar_t* adapter = nullptr;	 // a name reported by listGPUs, or nullptr for device 0
	};
	using pfnListAdapters = void ( * )( const wchar_t* name, void* pv );
	using pfnDecodedTokens = void ( * )( const int* tokens, int tokensLength, void* pv );

	using pfnLoadProgress = HRESULT ( * )( double val, void* pv ) noexcept;
	using pfnCancel = HRESULT ( * )( void* pv ) noexcept;
	struct sLoadModelCallbacks
	{
		pfnLoadProgress progress;
		pfnCancel cancel;
		void* pv;
	};

	enum struct eLogLevel : uint8_t { Error = 0, Warning = 1, Info = 2, Debug = 3 };
	enum struct eLoggerFlags : uint8_t { UseStandardError = 1, SkipFormatMessage = 2 };
	using pfnLoggerSink = void ( * )( void* context, eLogLevel lvl, const char* message );
	struct sLoggerSetup
	{
		pfnLoggerSink sink = nullptr;
		void* context = nullptr;
		eLogLevel level = eLogLevel::Warning;
		eLoggerFlags flags = (eLoggerFlags)0;
	};

	struct sLanguageEntry
	{
		uint32_t key;	 // up to 4 ASCII characters packed little-endian, see makeLanguageKey
		int id;
		const char* name;
	};
	struct sLanguageList
	{
		uint32_t length;
		const sLanguageEntry* pointer;
	};

	struct SpecialTokens
	{
		int TranscriptionEnd, TranscriptionStart, PreviousWord, SentenceStart, Not, TranscriptionBegin, TaskTranslate, TaskTranscribe;
	};

	// times are in 100-nanosecond ticks
	struct sTimeSpan { uint64_t ticks; };
	struct sTimeInterval { sTimeSpan begin, end; };
	struct sSegment
	{
		const char* text;
		sTimeInterval time;
		uint32_t firstToken, countTokens;
	};
	enum eTokenFlags : uint32_t { None = 0, Special = 1 };
	struct sToken
	{
		const char* text;
		sTimeInterval time;
		float probability, probabilityTimestamp, ptsum, vlen;
		int id;
		eTokenFlags flags;
	};
	struct sTranscribeLength { uint32_t countSegments, countTokens; };
	enum struct eResultFlags : uint32_t { None = 0, Tokens = 1, Timestamps = 2, NewObject = 0x100 };
	inline eResultFlags operator|( eResultFlags a, eResultFlags b ) { return (eResultFlags)( (uint32_t)a | (uint32_t)b ); }
	inline bool operator&( eResultFlags a, eResultFlags b ) { return 0 != ( (uint32_t)a & (uint32_t)b ); }
	enum struct eSpeakerChannel : uint8_t { Unsure = 0, Left = 1, Right = 2, NoStereoData = 0xFF };

	enum struct eSamplingStrategy : int { Greedy, BeamSearch };
	using pfnNewSegment = HRESULT ( * )( iContext* ctx, uint32_t n_new, void* user_data ) noexcept;
	using pfnEncoderBegin = HRESULT ( * )( iContext* ctx, void* user_data ) noexcept;	 // S_FALSE stops the run
	enum struct eFullParamsFlags : uint32_t
	{
		Translate = 1, NoContext = 2, SingleSegment = 4, PrintSpecial = 8, PrintProgress = 0x10, PrintRealtime = 0x20,
		PrintTimestamps = 0x40, TokenTimestamps = 0x100, SpeedupAudio = 0x200,
		// Extension (the bit is free in the reference's enum): token times from the decoder's cross-attention by dynamic time warping instead of the
		// TokenTimestamps heuristic (DESIGN.md "Token alignment"). Text tokens get t0 / t1 from the window's warping path, timestamp tokens their own time,
		// other special tokens the end of the token before them; vlen is what TokenTimestamps puts there, max_len wraps as under TokenTimestamps, and with
		// both flags set these times win. Needs no PCM: runStreamed takes it too. Greedy decoding of one stream only: beam search and iBatchRunner::run
		// answer E_NOTIMPL.
		AlignTokens = 0x1000,
	};
	inline eFullParamsFlags operator|( eFullParamsFlags a, eFullParamsFlags b ) { return (eFullParamsFlags)( (uint32_t)a | (uint32_t)b ); }

	struct sFullParams
	{
		eSamplingStrategy strategy;
		int cpuThreads;
		int n_max_text_ctx;
		int offset_ms;		// start offset in ms
		int duration_ms;	// audio duration to process in ms, 0 = all
		eFullParamsFlags flags;
		uint32_t language;
		float thold_pt, thold_ptsum;
		int max_len;
		int max_tokens;		// max tokens per segment, 0 = no limit
		struct { int n_past; } greedy;
		struct { int n_past, beam_width, n_best; } beam_search;
		int audio_ctx;		// overwrite the audio context size, 0 = default: the encoder takes 2 * audio_ctx frames per window, the decoder attends to audio_ctx keys
		const whisper_token* prompt_tokens;
		int prompt_n_tokens;
		pfnNewSegment new_segment_callback;
		void* new_segment_callback_user_data;
		pfnEncoderBegin encoder_begin_callback;
		void* encoder_begin_callback_user_data;

		bool flag( eFullParamsFlags f ) const { return 0 != ( (uint32_t)flags & (uint32_t)f ); }
		void resetFlag( eFullParamsFlags bit ) { flags = (eFullParamsFlags)( (uint32_t)flags & ~(uint32_t)bit ); }
		void setFlag( eFullParamsFlags bit, bool set = true )
		{
			uint32_t f = (uint32_t)flags;
			f = set ? ( f | (uint32_t)bit ) : ( f & ~(uint32_t)bit );
			flags = (eFullParamsFlags)f;
		}
	};

	inline uint32_t makeLanguageKey( const char* code )
	{
		uint32_t res = 0;
		for( uint32_t i = 0; i < 4 && code[ i ]; i++ ) res |= (uint32_t)(uint8_t)code[ i ] << ( 8 * i );
		return res;
	}

	using pfnReportProgress = HRESULT ( * )( double val, iContext* ctx, void* pv ) noexcept;
	struct sProgressSink
	{
		pfnReportProgress pfn;
		void* pv;
	};
	struct sCaptureDevice;
	// ---- audio capture (Whisper/API/MfStructs.h) ----
	enum struct eCaptureFlags : uint32_t
	{
		Stereo = 1,		// keep stereo PCM in addition to mono: detectSpeaker then works from the callbacks of a piece
		// Extension (the bit is free in the reference's enum): where the loop would post a piece while the previous one is still being transcribed, it waits
		// instead of growing the buffer and dropping samples; iPcmCapture::write then blocks instead of dropping. For a source that is not real time (a file, a pipe).
		NoDrop = 2,
	};
	// seconds; runCapture turns them into samples at 16 kHz, rounded to nearest even
	struct sCaptureParams
	{
		float minDuration = 2.0f;		   // a piece is not fired at a pause before it is this long; 0.125 .. 30
		float maxDuration = 3.0f;		   // a piece of continuous speech is fired at this length; 0.125 .. 30
		float dropStartSilence = 0.25f;	   // a buffer without any voice is dropped when it reaches this length
		float pauseDuration = 0.333f;	   // voice is "recent" when the last speech frame ended at most this long before the read
		uint32_t flags = 0;				   // eCaptureFlags
	};
	enum struct eCaptureStatus : uint8_t { Listening = 1, Voice = 2, Transcribing = 4, Stalled = 0x80 };
	// S_OK to continue, anything else to stop the capture session
	using pfnShouldCancel = HRESULT ( * )( void* pv ) noexcept;
	// called only when a bit changes, with the whole new word
	using pfnCaptureStatus = HRESULT ( * )( void* pv, eCaptureStatus status ) noexcept;
	struct sCaptureCallbacks
	{
		pfnShouldCancel shouldCancel;
		pfnCaptureStatus captureStatus;
		void* pv;
	};
	using pfnFoundCaptureDevices = HRESULT ( * )( int len, const sCaptureDevice* buffer, void* pv ) noexcept;

	// ---- interfaces ----------------------------------------------------------------------------------------------
	// {2871a73f-5ce3-48f8-8779-6582ee11935e}
	struct iTranscribeResult : public ComLight::IUnknown
	{
		static constexpr ComLight::GUID iid() { return { 0x2871a73f, 0x5ce3, 0x48f8, { 0x87, 0x79, 0x65, 0x82, 0xee, 0x11, 0x93, 0x5e } }; }
		virtual HRESULT getSize( sTranscribeLength& rdi ) const = 0;
		virtual const sSegment* getSegments() const = 0;
		virtual const sToken* getTokens() const = 0;
	};

	// {013583aa-c9eb-42bc-83db-633c2c317051}
	struct iAudioBuffer : public ComLight::IUnknown
	{
		static constexpr ComLight::GUID iid() { return { 0x013583aa, 0xc9eb, 0x42bc, { 0x83, 0xdb, 0x63, 0x3c, 0x2c, 0x31, 0x70, 0x51 } }; }
		virtual uint32_t countSamples() const = 0;
		virtual const float* getPcmMono() const = 0;
		virtual const float* getPcmStereo() const = 0;
		virtual HRESULT getTime( int64_t& rdi ) const = 0;
	};
	// {35b988da-04a6-476a-a193-d8891d5dc390}
	struct iAudioReader : public ComLight::IUnknown
	{
		static constexpr ComLight::GUID iid() { return { 0x35b988da, 0x04a6, 0x476a, { 0xa1, 0x93, 0xd8, 0x89, 0x1d, 0x5d, 0xc3, 0x90 } }; }
		virtual HRESULT getDuration( int64_t& rdi ) const = 0;
		virtual HRESULT getReader( IMFSourceReader** pp ) const = 0;
		virtual HRESULT requestedStereo() const = 0;
	};
	// {747752c2-d9fd-40df-8847-583c781bf013}
	struct iAudioCapture : public ComLight::IUnknown
	{
		static constexpr ComLight::GUID iid() { return { 0x747752c2, 0xd9fd, 0x40df, { 0x88, 0x47, 0x58, 0x3c, 0x78, 0x1b, 0xf0, 0x13 } }; }
		virtual HRESULT getReader( IMFSourceReader** pp ) const = 0;
		virtual const sCaptureParams& getParams() const = 0;
	};
	// Extension (no counterpart in the reference, whose captures are sound cards): a capture fed by the caller -- a pipe, a socket, its own code -- at 16 kHz or,
	// made by createPcmCaptureAtRate, at any rate from 1000 to 384000 Hz, which the capture buffer resamples chunk by chunk with the filter of the file path.
	// The only kind of capture iContext::runCapture of this library takes. write may be called from any thread while runCapture runs on another.
	// {3a9e5c72-1b4d-4f08-b6a1-7c2e9d5f8a13}
	struct iPcmCapture : public iAudioCapture
	{
		static constexpr ComLight::GUID iid() { return { 0x3a9e5c72, 0x1b4d, 0x4f08, { 0xb6, 0xa1, 0x7c, 0x2e, 0x9d, 0x5f, 0x8a, 0x13 } }; }
		// `frames` interleaved sample frames; format: 1 = signed 16 bit, 4 = 32 bit float (wh_pcm_format of whisper_hip.h); channels 1 or 2, the same in every
		// call. The chunk is queued as it is, a write of more than a second in pieces of a second; runCapture takes one queued chunk per read. While more than maxDuration + 1 s is queued: with eCaptureFlags::NoDrop
		// the call blocks until the loop has caught up, otherwise the OLDEST queued chunk is dropped and counted (droppedChunks). A chunk dropped here never
		// reaches the loop and is not part of the stream's sample clock: the times behind it are early by its length. E_INVALIDARG for another
		// format or channel count, E_UNEXPECTED after close.
		virtual HRESULT write( const void* samples, int format, int channels, uint32_t frames ) = 0;
		// the end of the stream: runCapture drains the queue, transcribes what is buffered if it holds voice, and returns S_OK
		virtual HRESULT close() = 0;
		virtual uint64_t droppedChunks() const = 0;
	};
	// {fb9763a5-d77d-4b6e-aff8-f494813cebd8}  -- on Linux: a WAV / raw-PCM loader stands in for Media Foundation
	struct iMediaFoundation : public ComLight::IUnknown
	{
		static constexpr ComLight::GUID iid() { return { 0xfb9763a5, 0xd77d, 0x4b6e, { 0xaf, 0xf8, 0xf4, 0x94, 0x81, 0x3c, 0xeb, 0xd8 } }; }
		virtual HRESULT loadAudioFile( LPCTSTR path, bool stereo, iAudioBuffer** pp ) const = 0;
		virtual HRESULT openAudioFile( LPCTSTR path, bool stereo, iAudioReader** pp ) = 0;
		virtual HRESULT loadAudioFileData( const void* data, uint64_t size, bool stereo, iAudioReader** pp ) = 0;
		virtual HRESULT listCaptureDevices( pfnFoundCaptureDevices pfn, void* pv ) = 0;
		virtual HRESULT openCaptureDevice( LPCTSTR endpoint, const sCaptureParams& captureParams, iAudioCapture** pp ) = 0;
	};

	// {b9956374-3b18-4943-90f2-2ab18a404537}
	struct iContext : public ComLight::IUnknown
	{
		static constexpr ComLight::GUID iid() { return { 0xb9956374, 0x3b18, 0x4943, { 0x90, 0xf2, 0x2a, 0xb1, 0x8a, 0x40, 0x45, 0x37 } }; }
		// PCM -> log-mel -> encoder -> greedy decoder -> segments, the complete model
		virtual HRESULT runFull( const sFullParams& params, const iAudioBuffer* buffer ) = 0;
		virtual HRESULT runStreamed( const sFullParams& params, const sProgressSink& progress, const iAudioReader* reader ) = 0;
		virtual HRESULT runCapture( const sFullParams& params, const sCaptureCallbacks& callbacks, const iAudioCapture* reader ) = 0;
		virtual HRESULT getResults( eResultFlags flags, iTranscribeResult** pp ) const = 0;
		virtual HRESULT detectSpeaker( const sTimeInterval& time, eSpeakerChannel& result ) const = 0;
		virtual HRESULT getModel( iModel** pp ) = 0;
		virtual HRESULT fullDefaultParams( eSamplingStrategy strategy, sFullParams* rdi ) = 0;
		virtual HRESULT timingsPrint() = 0;
		virtual HRESULT timingsReset() = 0;
	};

	// {abefb4c9-e8d8-46a3-8747-5afbadef1adb}
	struct iModel : public ComLight::IUnknown
	{
		static constexpr ComLight::GUID iid() { return { 0xabefb4c9, 0xe8d8, 0x46a3, { 0x87, 0x47, 0x5a, 0xfb, 0xad, 0xef, 0x1a, 0xdb } }; }
		virtual HRESULT createContext( iContext** pp ) = 0;
		virtual HRESULT tokenize( const char* text, pfnDecodedTokens pfn, void* pv ) = 0;
		virtual HRESULT isMultilingual() = 0;
		virtual HRESULT getSpecialTokens( SpecialTokens& rdi ) = 0;
		virtual const char* stringFromToken( whisper_token token ) = 0;
		virtual HRESULT clone( iModel** rdi ) = 0;
	};

	// ---- the seven exports of Whisper.dll (Whisper/whisper.def) ---------------------------------------------------
	WHISPER_EXPORT HRESULT setupLogger( const sLoggerSetup& setup );
	WHISPER_EXPORT HRESULT loadModel( const wchar_t* path, const sModelSetup& setup, const sLoadModelCallbacks* callbacks, iModel** pp );
	// Extension (no counterpart in whisper.def): one process per GPU. whComm is a wh_comm* of include/whisper_hip.h; rank `root`
	// reads the tensors, the other ranks receive the weight arena over RCCL and read only the header of the file.
	WHISPER_EXPORT HRESULT loadModelShared( const wchar_t* path, const sModelSetup& setup, const sLoadModelCallbacks* callbacks, void* whComm, int root, iModel** pp );
	// Extension (no counterpart in whisper.def): K recordings -- or K pieces of recordings -- transcribed in LOCK STEP on one GPU.
	// Every stream keeps the semantics of iContext::runFull on its own (ContextImpl.cpp:452-793: seek by the last timestamp, prompt
	// carry-over unless NoContext, stop rules, failure handling, callbacks on the calling thread), and its transcript is the transcript
	// runFull gives for the same samples; what changes is the device work: the next windows of up to `maxSlots` streams are ONE encoder
	// batch and ONE decode chain (a decode step costs about the same for 1 and for 64 sequences), `groups` such batches are in flight
	// on separate HIP streams (the encoder of one runs under the decode chain of the other), and a slot whose stream has finished is
	// refilled with the next stream. The reference's nearest facilities: whisper_full_parallel (Whisper/source/whisper.cpp:3127) and
	// iModel::clone + one iContext per thread (Whisper/Whisper/ModelImpl.cpp:40-60).
	struct sBatchStream
	{
		// Samples [firstSample, firstSample + countSamples) of the buffer's mono PCM (16 kHz), transcribed as a recording of its own:
		// its spectrogram is normalised on its own maximum and windows never read past its end -- how independent 30 s chunks of one
		// recording are declared. countSamples 0 = to the end of the buffer. Segment and token times are relative to the BUFFER
		// (the stream's first sample adds firstSample / 16000 s), plus the buffer's media time (iAudioBuffer::getTime).
		const iAudioBuffer* buffer;
		int64_t firstSample, countSamples;
		const sFullParams* params;	  // nullptr = the call's common parameters (callbacks receive a per-stream iContext: getResults, getModel)
	};
	struct sBatchSetup
	{
		uint32_t maxSlots;		// streams per lock-step batch (the device contexts are sized for it); 0 = 64, at most 512
		uint32_t groups;		// lock-step batches in flight; 0 = 2
		uint32_t greedyChunk;	// greedy steps enqueued at a time; 0 = 4. The host applies its stop rules chunk by chunk, so up to one chunk is decoded past the end of a round
		uint32_t flags;			// 1 = keep one more chunk queued behind the one in flight (the device never waits for the host; up to two chunks are decoded in vain)
	};
	// {6f0c9a1e-3b52-4d7c-8e21-9a4f5c7d2b10}
	struct iBatchRunner : public ComLight::IUnknown
	{
		static constexpr ComLight::GUID iid() { return { 0x6f0c9a1e, 0x3b52, 0x4d7c, { 0x8e, 0x21, 0x9a, 0x4f, 0x5c, 0x7d, 0x2b, 0x10 } }; }
		// results[i] receives the transcript of streams[i] (a new object, the caller releases it; nullptr when the stream failed before it
		// produced one). Returns the first failure of any stream, S_OK otherwise; perStream, when non-null, receives every stream's own
		// HRESULT (S_FALSE: shorter than a second, an empty transcript -- runFull's S_FALSE). Not re-entrant; callbacks of sFullParams
		// arrive on the calling thread and receive a per-stream iContext (getResults, getModel).
		virtual HRESULT run( const sFullParams& params, const sBatchStream* streams, uint32_t count, iTranscribeResult** results, HRESULT* perStream ) = 0;
	};
	// The runner owns the device contexts of its groups (KV caches for maxSlots windows each, captured decode graphs): a service creates
	// it once. runFullBatch = createBatchRunner + run + Release for a one-off call.
	WHISPER_EXPORT HRESULT createBatchRunner( iModel* model, const sBatchSetup* setup, iBatchRunner** pp );
	WHISPER_EXPORT HRESULT runFullBatch( iModel* model, const sFullParams& params, const sBatchStream* streams, uint32_t count, const sBatchSetup* setup,
		iTranscribeResult** results, HRESULT* perStream );
	// The decoder heads whose cross-attention weights the AlignTokens flag averages, for every context of the model: `count` (layer, head) pairs, used in
	// ascending (layer, head) order. count == 0 restores the default, every head of the upper half of the decoder's layers (what openai-whisper takes for a
	// model that names none). A free function: iModel's vtable is the reference's. E_INVALIDARG for a pair outside the model or a model of another library.
	WHISPER_EXPORT HRESULT setAlignmentHeads( iModel* model, const int32_t* layerHeadPairs, uint32_t count );
	// Extension (the reference has no temperature and no quality gate anywhere in Whisper/API): decoding fallback, as openai-whisper and whisper.cpp do it, for one
	// stream through iContext::runFull / runStreamed with the Greedy strategy. A window's greedy attempt is scored over its resultLen tokens -- avgLogprob = the
	// mean of ln max( p, FLT_MIN ), entropy = that of the token ids among the last 32 -- and fails when the stop rules call it failed, when it is empty, when
	// avgLogprob < logprobThold, or when it is longer than 32 tokens and entropy < entropyThold. A failed attempt is decoded again (no second encode) by sampling at
	// temperature k * temperatureInc, k = 1, 2, ... up to 1.0; the last attempt stands whatever its scores. An attempt the stop rules did not fail whose window has
	// P( <|nospeech|> ) > noSpeechThold and avgLogprob < logprobThold is skipped instead: no segments, no prompt carry-over, the stream moves on. The rules are
	// DESIGN.md section 7; whisper_amd/host/decodeFallback.h holds them. A free function: iContext's vtable is the reference's. nullptr = off, the state of every
	// new context: the transcript of a run with the feature off is what it always was. With it on, eSamplingStrategy::BeamSearch answers E_NOTIMPL; the batch
	// runner has its own switch, setBatchDecodingFallback below. E_INVALIDARG for a context of another library, a NaN threshold, or 0 < temperatureInc < 0.01.
	struct sDecodingFallback
	{
		float temperatureInc = 0.2f;	// <= 0: one greedy attempt, gates only
		float logprobThold = -1.0f;
		float entropyThold = 2.4f;
		float noSpeechThold = 0.6f;
		uint64_t seed = 0;				// the draws of a run are a function of ( seed, window, attempt, position )
	};
	WHISPER_EXPORT HRESULT setDecodingFallback( iContext* context, const sDecodingFallback* params );
	// What the fallback did with each window of the context's last run, in order (a window the stop rules made the stream retry appears once per visit)
	struct sWindowStats
	{
		int32_t seek;			// the window's first frame, 10 ms units
		int32_t attempts;
		float temperature;		// of the last attempt
		float noSpeech;
		double avgLogprob, entropy;	  // of the last attempt
		uint32_t skipped;		// 1: the silence rule dropped the window
		uint32_t reserved;
	};
	// count in: the capacity of `stats`; out: the number of windows (stats may be nullptr to ask for it). Empty when the run had the feature off.
	WHISPER_EXPORT HRESULT getWindowStats( const iContext* context, sWindowStats* stats, uint32_t* count );
	// The same feature for the lock-step batch runner: every later run of the runner scores each stream's windows with the rules above. A window whose attempt
	// fails STAYS in its slot -- same seek, same prompt -- and is decoded again in its group's next round at the next temperature while its neighbours move on
	// to new windows: a retried window costs one slot-round (a round encodes and decodes every slot whatever it holds), and the rows of one decode step sample
	// each under its own temperature, key and nonce (wh_context_set_sampling_rows). The draws of stream i use the key seed + i: the chunks of one recording all
	// stand at seek 0 and must not share draws. A stream's transcript does not depend on its neighbours' retries; with gates that never fire it is the transcript
	// of the runner with the feature off. With maxSlots <= 4 a greedy row of a round in which a neighbour retries is sampled by another kernel than in an
	// all-greedy round (the spread sampler has no per-row form): its ptsum may then differ in the last bits of a double sum. A stream whose every window was skipped as silence ends
	// with S_FALSE in perStream and an empty result, like a recording too short to transcribe. nullptr = off, the state of every
	// new runner. E_INVALIDARG as setDecodingFallback; E_NOTIMPL where the scheduler was built without the device's per-row sampler. BeamSearch and AlignTokens
	// in a batch stay E_NOTIMPL.
	WHISPER_EXPORT HRESULT setBatchDecodingFallback( iBatchRunner* runner, const sDecodingFallback* params );
	// What the fallback did with each window of the stream a batch runner's result object belongs to, in order; count as getWindowStats. Empty with the feature off.
	WHISPER_EXPORT HRESULT getResultWindowStats( const iTranscribeResult* result, sWindowStats* stats, uint32_t* count );
	// Extension: suppressed tokens, openai-whisper's definition -- the logits of the given token ids are replaced by -inf before the softmax, so the decoder can
	// never emit them, whatever the strategy: greedy runs, the sampled attempts of the decoding fallback, eSamplingStrategy::BeamSearch. Free functions: the
	// vtables are the reference's. The ids are text tokens, each in [ 0, eot ): eot, the task and language tokens and the timestamps cannot be suppressed.
	// getNonSpeechTokens: the set openai-whisper suppresses by default (suppress_tokens = "-1") and whisper.cpp under --suppress-nst -- brackets, quotes that open a
	// word, note symbols, "((", "[[", "♪♪" and the like -- found by exact match in the model's own vocabulary (whisper_amd/host/nonSpeechTokens.h), ascending.
	// count in: the capacity of `ids`; out: the size of the set (ids may be nullptr to ask for it); E_BOUNDS when the capacity is too small.
	WHISPER_EXPORT HRESULT getNonSpeechTokens( iModel* model, int32_t* ids, uint32_t* count );
	// The set holds for every later runFull / runStreamed of the context and reaches every device context it owns or creates later. count == 0 = off, the state of
	// every new context: such a run is what it always was. Language "auto" detects on the unfiltered distribution as before; prompt tokens are fed, not sampled,
	// so a suppressed id in prompt_tokens is legal. With a set held the no-speech probability of the decoding fallback is that of the filtered distribution.
	// E_INVALIDARG for an id outside [ 0, eot ) or a context of another library.
	WHISPER_EXPORT HRESULT setSuppressedTokens( iContext* context, const int32_t* ids, uint32_t count );
	// One set for all streams of every later run of the runner. E_INVALIDARG as above; E_NOTIMPL for a non-empty set where the scheduler was built without the
	// device's logit filter.
	WHISPER_EXPORT HRESULT setBatchSuppressedTokens( iBatchRunner* runner, const int32_t* ids, uint32_t count );
	// Extension: timestamp rules, the three clauses of openai-whisper's ApplyTimestampRules (whisper.cpp: whisper_process_logits) the sampler does not hold, applied
	// to the logits on the device in every step of the decoding loop: after `text, <|t|>` a timestamp or eot follows, after `<|t|>, <|t|>` no timestamp; no timestamp
	// lies below the last one of its window; a segment has non-zero length. With them on, the host loop no longer meets a timestamp that goes back in time, which it
	// answers by cutting the window there. They hold for greedy runs and for the sampled attempts of the decoding fallback. Off unless set: such a run is what it
	// always was. Free functions: the vtables are the reference's. With the rules on, a run with eSamplingStrategy::BeamSearch answers E_NOTIMPL (the per-sequence
	// history would have to follow the beam's reorder); language detection and eFullParamsFlags::AlignTokens read unfiltered passes as before.
	// E_INVALIDARG for a context of another library.
	WHISPER_EXPORT HRESULT setTimestampRules( iContext* context, bool on );
	// One switch for all streams of every later run of the runner. E_NOTIMPL to turn it on where the scheduler was built without the device's filter.
	WHISPER_EXPORT HRESULT setBatchTimestampRules( iBatchRunner* runner, bool on );
	// Extension: phrase boosting ("hotwords", contextual biasing) -- the caller names phrases, as rows of text-token ids, and one boost; in every step of the
	// decoding loop the boost is added on the device to the logit of every token that continues a phrase after what the stream has just emitted (the text tokens
	// since its last timestamp; the start of a phrase is always offered), before the softmax. DESIGN.md section 7 "Phrase boosting" holds the definition. It
	// applies to greedy runs and to the sampled attempts of the decoding fallback, each attempt from an empty history. Suppressed tokens and the timestamp rules
	// win (-inf stays -inf). The probabilities a run reports, and what the fallback's gates see, are the boosted distribution's. A partial match keeps its bonus.
	// There is NO default boost: a useful value on a real checkpoint has not been measured, and neither has recognition accuracy with boosting on.
	// Off unless set: such a run is what it always was. Free functions: the vtables are the reference's.
	struct sBoostedPhrases
	{
		const int32_t* tokens;	   // [ count ][ maxLength ]: row p holds lengths[ p ] ids, each in [ 0, eot )
		const int32_t* lengths;	   // [ count ], each 1 .. 16 and <= maxLength
		uint32_t count;			   // at most 1024; 0 = off
		uint32_t maxLength;
		float boost;			   // finite, > 0: added to the logits
	};
	// The set holds for every later runFull / runStreamed of the context. nullptr or count == 0 = off, the state of every new context. With a set held, a run
	// with eSamplingStrategy::BeamSearch answers E_NOTIMPL (the per-sequence state would have to follow the beam's reorder); language detection,
	// eFullParamsFlags::AlignTokens and scoreTokens read unboosted passes. E_INVALIDARG for an id outside [ 0, eot ), a boost that is NaN, infinite or not
	// positive, more than 1024 phrases, a phrase of 0 or more than 16 tokens, tables beyond the device's cap, or a context of another library.
	WHISPER_EXPORT HRESULT setBoostedPhrases( iContext* context, const sBoostedPhrases* phrases );
	// One set for all streams of every later run of the runner. E_INVALIDARG as above; E_NOTIMPL for a non-empty set where the scheduler was built without the
	// device's filter.
	WHISPER_EXPORT HRESULT setBatchBoostedPhrases( iBatchRunner* runner, const sBoostedPhrases* phrases );
	// Extension: no-repeat n-grams, Hugging Face generation's no_repeat_ngram_size restricted to text tokens, applied to the logits on the device in every step of
	// the decoding loop. n = 0: off, the state of every new context; 1 .. 8: a text token cannot be sampled when it would complete an n-gram that the tokens sampled
	// in the current window, timestamps included, already hold. eot and the timestamps are never forbidden, the prompt does not count, and no history survives into
	// the next window. It holds for greedy runs and for the sampled attempts of the decoding fallback. There is no default n. With n != 0 a run with
	// eSamplingStrategy::BeamSearch answers E_NOTIMPL (the per-sequence history would have to follow the beam's reorder); language detection, scoring and
	// eFullParamsFlags::AlignTokens read unfiltered passes as before. E_INVALIDARG for n outside 0 .. 8 and for a context of another library.
	WHISPER_EXPORT HRESULT setNoRepeatNgram( iContext* context, int n );
	// One n for all streams of every later run of the runner. E_INVALIDARG as above; E_NOTIMPL for n != 0 where the scheduler was built without the device's filter.
	WHISPER_EXPORT HRESULT setBatchNoRepeatNgram( iBatchRunner* runner, int n );
	// One text phrase as rows for sBoostedPhrases: the text as written and, when it does not begin with a space, also the text behind one space, which is how a
	// word is spelled in mid-sentence; rows that come out equal collapse. tokens [ cap ][ 16 ], lengths [ cap ]; count in: cap, out: the rows written (1 or 2);
	// E_BOUNDS when cap is too small. E_INVALIDARG, the log naming the phrase, when a spelling is empty or longer than 16 tokens.
	WHISPER_EXPORT HRESULT phraseSpellings( iModel* model, const char* text, int32_t* tokens, int32_t* lengths, uint32_t* count );
	// Extension: scoring a GIVEN transcript -- "how probable is this text for this audio?" -- and, with flag 1, forced alignment of a known text. The tokens are
	// fed to the decoder (teacher forcing) and every scored token receives its log-probability under the model's OWN distribution: neither suppressed tokens nor
	// the timestamp rules nor the sampler's clauses apply, and a context's decoding settings do not matter. True logarithms (an unlikely token scores a large
	// negative number, not -inf); the definition is wh_token_score's in whisper_hip.h. Free functions: the vtables are the reference's.
	struct sScoreRequest
	{
		// samples [firstSample, firstSample + countSamples) of the buffer's mono PCM (16 kHz); countSamples 0 = to the end. A clip of 1 to 30 s: its spectrogram is
		// the one runFull makes of those samples, normalised on its own maximum, scored as ONE window at seek 0 with the model's full audio context. Anything
		// shorter or longer is E_INVALIDARG: long-form scoring (walking the windows of a recording) is out of scope.
		const iAudioBuffer* buffer;
		int64_t firstSample, countSamples;
		const whisper_token* prompt;	// fed, not scored: [prev + past text,] sot, language, task[, no-timestamps] (makeSotSequence)
		uint32_t promptCount;
		const whisper_token* tokens;	// scored; eot is appended and scored too: count + 1 records
		uint32_t count;
		uint32_t flags;					// 1 = also align (forced alignment): the prompt must hold the no-timestamps token exactly once and as its last entry, the
										// scored tokens must all lie below eot; promptCount + count + 1 <= min( 256, n_text_ctx ) in any case
	};
	struct sTokenScore
	{
		float logprob, bestLogprob;		// of the token, and of the arg-max of its row
		int32_t best, rank;				// the arg-max (ties to the lower id); how many ids the model prefers to the token (0 = it is what greedy decoding takes)
		sTimeInterval time;				// flag 1: from the warping path, by the frame-to-time rule of eFullParamsFlags::AlignTokens (eot: the end of the text),
										// relative to the buffer plus its media time; zero without the flag (timestamp tokens among the scored tokens are then legal)
	};
	// scores: request.count + 1 records. Uses the context's own device context: its self-attention caches are overwritten, its results and settings stay.
	// E_INVALIDARG for a context of another library, an empty prompt or token list, an id outside the vocabulary, a row that is too long, a clip outside 1 .. 30 s.
	WHISPER_EXPORT HRESULT scoreTokens( iContext* context, const sScoreRequest& request, sTokenScore* scores );
	// `count` requests on the runner's first group, up to maxSlots per pass in request order; one pass = one encoder batch and one scoring call. scores[ i ]:
	// requests[ i ].count + 1 records. perRequest, when non-null, receives every request's own HRESULT; returns the first failure, S_OK otherwise: a request that
	// fails its checks does not keep its neighbours from being scored. Flag 1 is E_NOTIMPL here (token alignment in a batch runner is). E_NOTIMPL where the
	// scheduler was built without the device's scorer.
	WHISPER_EXPORT HRESULT scoreBatch( iBatchRunner* runner, const sScoreRequest* requests, uint32_t count, sTokenScore* const* scores, HRESULT* perRequest );
	// The tokens that select the task, as runFull builds them: sot[, language, transcribe | translate] for a multilingual model, then the no-timestamps token unless
	// `timestamps`. language: makeLanguageKey( "en" ). count in: the capacity of `out`; out: the number of tokens (E_BOUNDS when the capacity is too small).
	WHISPER_EXPORT HRESULT makeSotSequence( iModel* model, uint32_t language, bool translate, bool timestamps, whisper_token* out, uint32_t* count );
	// Extension (no counterpart in whisper.def): ONE long recording onto the batched path. The buffer is cut into pieces of at most maxLen samples at pauses,
	// found with the reference's voice-activity detector (Whisper/Whisper/voiceActivityDetection.cpp, which its capture loop uses to fire a transcription when
	// the speaker pauses): the per-frame features come from the device (wh_vad_features of whisper_hip.h, on the calling thread's current device), the decision
	// and the plan are host code. A cut lies in the middle of a pause of at least pauseFrames frames of 256 samples, the last such pause that leaves the piece
	// between minLen and maxLen samples; without one, where 21 frames hold the least energy. The plan is a partition of the buffer and a function of the samples
	// alone. Run the pieces with NoContext: they are independent recordings.
	struct sSplitParams
	{
		int64_t maxLen, minLen;		// samples; 0 = 480000 (30 s: a piece is one window) and 240000. 16000 <= minLen <= maxLen - 32000, maxLen <= 480000
		uint32_t pauseFrames;		// 0 = 21 (0.336 s; the reference's pauseDuration is 0.333 s)
		uint32_t reserved;
	};
	// receives the pieces as ready streams over the buffer (params nullptr = the call's common parameters), valid during the call; its result is splitAtPauses's
	using pfnSplitChunks = HRESULT ( * )( const sBatchStream* streams, uint32_t count, void* pv );
	WHISPER_EXPORT HRESULT splitAtPauses( const iAudioBuffer* buffer, const sSplitParams* params /* nullptr = defaults */, pfnSplitChunks pfnChunks, void* pv );
	// Extension: speech only -- what faster-whisper calls vad_filter and whisper.cpp --vad. The run finds the speech with the voice-activity detector above,
	// transcribes only that, and reports every time on the recording's own clock. It acts where the samples are in device memory already: the features are
	// computed on the uploaded buffer (wh_vad_features), 12 bytes per 256-sample frame go to the host for the decision, the spans go back, one kernel packs the
	// kept samples (wh_speech_pack) and the spectrogram is taken from the packed buffer; the decoding loop runs on it unchanged, so every strategy and every
	// decoding option works as before. The rules (whisper_amd/host/speechSpans.h; DESIGN.md section 7 "Speech only"), on the detector's per-frame flags:
	// maximal runs of speech frames; neighbours closer than minSilenceFrames merge; merged runs shorter than minSpeechFrames are dropped; each run grows by
	// padFrames on both sides (clamped; runs that now touch merge); a run that reaches the last whole frame takes the partial frame behind it. The defaults
	// are faster-whisper's vad_filter values rounded to frames; nobody has measured them for this detector on real speech.
	// Times: a segment's and a token's begin maps by the start rule (packed position s of span i -> a_i + s - out_i), an end by the end rule (the start rule of
	// s - 1, plus 1), so a segment that ends exactly at a join ends where the earlier span ends; a segment that straddles a join keeps the gap inside it.
	// Speakers (detectSpeaker, the per-segment speakers) are answered on the caller's stereo PCM at the mapped times.
	struct sSpeechFilter
	{
		int32_t minSilenceFrames;	// frames of 256 samples (16 ms); 0 = 125 (2.0 s)
		int32_t minSpeechFrames;	// 0 = 16 (0.256 s)
		int32_t padFrames;			// 0 = 25 (0.4 s)
		uint32_t flags;				// reserved, 0
	};
	struct sSpeechSpan { int64_t firstSample, endSample; };	  // [firstSample, endSample) at 16 kHz
	// Holds for every later runFull / runStreamed of the context; nullptr = off, the state of every new context: such a run allocates, launches and computes what
	// it always did. No speech at all: S_OK, no segments, one Info line, nothing encoded. Less than a second of speech: S_FALSE, like a recording that short.
	// One span that covers the recording: the unfiltered run, bit for bit. While the filter is on, a run with non-zero offset_ms or duration_ms answers
	// E_INVALIDARG and one with eFullParamsFlags::TokenTimestamps E_NOTIMPL (its stamper reads the host's PCM); runCapture ignores the filter (its pieces are
	// fired by the same detector already). E_INVALIDARG for a parameter that is negative or above 2^20, non-zero flags, or a context of another library.
	WHISPER_EXPORT HRESULT setSpeechFilter( iContext* context, const sSpeechFilter* params );
	// The spans the context's last runFull / runStreamed used. count in: the capacity of `spans`; out: the number of spans (spans may be nullptr to ask for it);
	// E_BOUNDS when the capacity is too small. Empty when the run had the filter off -- and when it found no speech.
	WHISPER_EXPORT HRESULT getSpeechSpans( const iContext* context, sSpeechSpan* spans, uint32_t* count );
	// The spans alone, the counterpart of splitAtPauses: features on the calling thread's current device, decision and rules on the host. pfnSpans receives
	// them, ascending and disjoint, valid during the call; its result is speechSpans's.
	using pfnSpeechSpans = HRESULT ( * )( const sSpeechSpan* spans, uint32_t count, void* pv );
	WHISPER_EXPORT HRESULT speechSpans( const iAudioBuffer* buffer, const sSpeechFilter* params /* nullptr = defaults */, pfnSpeechSpans pfnSpans, void* pv );
	// The same switch for the lock-step batch runner: every stream of every later run is filtered when it is admitted, on the device context that uploads it;
	// its times are mapped with its own map before its own offset in the buffer is added. A stream without speech gets an empty result and S_OK and never
	// takes a slot. The pieces splitAtPauses plans are filtered one by one, so silent pieces are dropped and the ends of the others trimmed.
	// E_NOTIMPL where the scheduler was built without the device's packer.
	WHISPER_EXPORT HRESULT setBatchSpeechFilter( iBatchRunner* runner, const sSpeechFilter* params );
	// The spans the stream behind a batch runner's result object used, relative to the stream's first sample; count as getSpeechSpans.
	WHISPER_EXPORT HRESULT getResultSpeechSpans( const iTranscribeResult* result, sSpeechSpan* spans, uint32_t* count );
	// Extension: live transcription. iContext::runCapture runs the reference's capture loop (Whisper/Whisper/ContextImpl.capture.cpp; DESIGN.md section 7 "Live
	// capture") over an iPcmCapture: every piece the loop fires is a runFull on a worker thread of the library, with the buffer's media time set to the piece's
	// first sample, so segment times are stream times and the context's decoding options apply to every piece. OS capture devices (listCaptureDevices,
	// openCaptureDevice) stay E_NOTIMPL.
	// createPcmCaptureAtRate: what is written has `sampleRate` frames per second, 1000 .. 384000 or E_INVALIDARG; createPcmCapture means 16000. At another rate
	// than 16000 every chunk is resampled to 16 kHz on the device by the launch that looks for voice in it, with the resampler of the file path made resumable:
	// the 16 kHz samples the loop sees are, bit for bit, those the file path gives for the whole stream at once, whatever the chunk sizes. The durations of
	// sCaptureParams, the pieces' start samples and the segment times are those of the 16 kHz stream. The filter looks ahead half + 1 input frames (2.1 to 2.2 ms
	// from 22.05 kHz up, 4.4 ms at 8 kHz): a sample reaches the loop that much later. Reads discarded while the loop is stalled count as silence for the filter.
	WHISPER_EXPORT HRESULT createPcmCapture( const sCaptureParams& params, iPcmCapture** pp );
	WHISPER_EXPORT HRESULT createPcmCaptureAtRate( const sCaptureParams& params, uint32_t sampleRate, iPcmCapture** pp );
	WHISPER_EXPORT HRESULT initMediaFoundation( iMediaFoundation** pp );
	WHISPER_EXPORT uint32_t findLanguageKeyW( const wchar_t* lang );
	WHISPER_EXPORT uint32_t findLanguageKeyA( const char* lang );
	WHISPER_EXPORT HRESULT getSupportedLanguages( sLanguageList& rdi );
	WHISPER_EXPORT HRESULT listGPUs( pfnListAdapters pfn, void* pv );
}

// Flat C mirror of the above for FFI callers that cannot consume C++ vtables (ctypes, cgo ...): whisper_c.h
