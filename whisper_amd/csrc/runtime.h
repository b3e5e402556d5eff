// Private declarations of the runtime behind the C ABI of include/whisper_hip.h: the model arena, the context and what the units
// options / model / comm / context / encode / exact_graphs / step_graph / decode / beam / ops_debug (.hip) share.
//
// The runtime is the MI355X counterpart of the reference's DirectCompute::WhisperContext
// (Whisper/Whisper/WhisperContext.cpp: encode :310-399, encodeLayer :158-289, decode :578-639, decodeLayer :407-576),
// ModelBuffers (Whisper/Whisper/ModelBuffers.h:8-112) and KeyValueBuffers (KeyValueBuffers.h:7-53). It is host code
// only: every arithmetic step is a kernel from gemm*.hip / attn_enc.hip / attn_dec.hip / elementwise.hip / sample.hip / mel.hip
// (beam.hip keeps the beam ranking and the cache reorder next to its entry points, filters.hip the logit filters next to their owner).
//
// Memory model (sized for 288 GB of HBM3E, no allocation in steady state):
//   * ONE packed weight arena per model, layout a pure function of the hparams, so a rank that did not read the file
//     can receive it with a single RCCL broadcast. Q/K/V weights of a layer are concatenated to one [3d][d] matrix, the
//     cross-attention K/V weights of ALL decoder layers to one [2*L*d][d] matrix (one big GEMM per window).
//   * per context: activations for maxBatch windows in lock step + FP16 KV caches
//       cross  [layer][batch][head][n_audio_ctx][64]   (K pre-scaled by (d/H)^-0.25, whisper.cpp:1465)
//       self   [layer][batch][head][n_text_ctx][64]
#pragma once
#include "kernels.h"
#include "../../include/whisper_hip.h"
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <condition_variable>
#include <memory>
#include <cstdlib>
#include <functional>
#include <set>
#include <string>
#include <vector>
#include <chrono>
#include <dlfcn.h>
#include <atomic>
#include <thread>

namespace wh
{
	inline int roundUp( int x, int m ) { return ( x + m - 1 ) / m * m; }
	// conv1 as an implicit GEMM: K = 3 taps * n_mels channels, zero-padded to a multiple of 64 (80 mels: 240 -> 256;
	// the 128 mels of the large-v3 shape: 384 exactly)
	constexpr int CONV1_KPAD_MAX = 512;
	inline int conv1Kpad( const wh_hparams& hp ) { return roundUp( 3 * hp.n_mels, 64 ); }

	// Special token ids follow from the vocabulary size (Whisper/Whisper/Vocabulary.h:27-41 hard-codes 51864 / 51865):
	// every language token added to the multilingual vocabulary moves the ids behind the language block up by one.
	// 51864 (.en) -> extra 0, 51865 (multilingual, 99 languages) -> 1, 51866 (the large-v3 shape, 100 languages) -> 2.
	struct SpecialIds { int sot, solm, tnot, beg; };
	inline SpecialIds specialIds( const wh_hparams& hp )
	{
		const int extra = hp.n_vocab > 51864 ? hp.n_vocab - 51864 : 0;
		return SpecialIds{ 50257 + ( extra > 0 ? 1 : 0 ), 50361 + extra, 50362 + extra, 50363 + extra };
	}

	struct EncLayer
	{
		int64_t ln1w, ln1b, wqkv, bqkv, wo, bo, ln2w, ln2b, w1, b1, w2, b2;
	};
	struct DecLayer
	{
		int64_t ln1w, ln1b, wqkv, bqkv, wo, bo, lncw, lncb, wcq, bcq, wco, bco, ln2w, ln2b, w1, b1, w2, b2;
	};
	struct Layout
	{
		int64_t filters, dft, expTab, encPe, conv1w, conv1b, conv2w, conv2b, lnPostW, lnPostB;
		int64_t decPe, te, decLnW, decLnB, wcross, bcross;
		std::vector<EncLayer> enc;
		std::vector<DecLayer> dec;
		int64_t total;
	};

	// One device buffer of an owner: a context's `allocations`, the registry of wh_buffer_alloc (name == nullptr). With WH_DEBUG_POISON
	// set it has a guard region on both sides of the body; otherwise base == body.
	struct Allocation { void* base; void* body; int64_t bytes; const char* name; };
	// hipMalloc, guard fill, and the body filled with the byte `fill` (negative: left as allocated); the fills are ordered on `stream`
	hipError_t guardedAlloc( Allocation& a, int64_t bytes, int fill, const char* name, hipStream_t stream );
	// Guard regions intact? Violations go to stderr with the buffer's name and the first damaged offset (negative = before the body).
	// Then hipFree. Returns the number of damaged guards, or WH_E_HIP when the free failed.
	int guardedFree( const Allocation& a );
}	// namespace wh
using namespace wh;

struct wh_model
{
	wh_hparams hp;
	Layout L;
	uint8_t* arena = nullptr;
	bool ownsArena = false;
	bool finalized = false;
	std::set<std::string> loaded;
	bool filtersSet = false;
	Allocation staging = { nullptr, nullptr, 0, nullptr };	   // raw blocks of the quantized tensor being loaded; freed by wh_model_finalize / wh_model_destroy
	int device = 0;	   // the HIP device the arena lives on; every entry point binds the calling thread to it
	std::vector<int32_t> alignHeads;	   // wh_model_set_alignment_heads: (layer, head) pairs, ascending; empty = every head of the upper half of the decoder
	template<class T> T* at( int64_t off ) const { return (T*)( arena + off ); }
	size_t expectedTensors() const { return 11 + 15 * (size_t)hp.n_audio_layer + 24 * (size_t)hp.n_text_layer; }
};

// HIP's current device is per host thread. The reference binds the model's device to the calling thread at the top of
// every call (Device::setForCurrentThread, Whisper/ML/Device.cpp:163-177); so do we, which is what lets a context be
// created or run from a thread other than the one that loaded the model (iModel::clone, sModelSetup.adapter).
namespace wh { int bindDevice( const wh_model* m ); }
#define WH_BIND( model ) WH_CHECK( bindDevice( model ) )

// Per-kernel-class GPU timing, the counterpart of the reference's GpuProfiler (Whisper/Utils/GpuProfiler.h:21-188: a
// timestamp query per shader dispatch, aggregated per eComputeShader). hipEvent pairs on the context's stream; only
// active between wh_profile_enable(1) and wh_profile_read, because two event records per launch perturb launch-bound code.
enum eKernelClass : int
{
	KC_GEMM_TILED = 0, KC_GEMM_SKINNY, KC_GEMV, KC_ATTN_ENC, KC_ATTN_DEC, KC_ATTN_DEC_CROSS, KC_SELF_BLOCK, KC_LAYER_NORM, KC_MEL, KC_MEL_TO_CONV, KC_EMBED, KC_SOFTMAX,
	KC_SAMPLE, KC_EVENT_PAIR, KC_LAYER_NORM_DEC, KC_GEMM_DEC, KC_COUNT
};
// "attentionDecCross" = cross-attention launches (attentionDecG<NQ, true> / <NQ, false> with group or nKeys = n_audio_ctx),
// "attentionDec" = causal self-attention; "eventPair" = the calibration launches of wh_profile_enable (an empty kernel
// between the same two event records: what the bracket itself costs, to be subtracted from every per-launch average).
static const char* const kernelClassNames[ KC_COUNT ] = { "gemmTiled", "gemmSkinny", "gemvFused", "attentionEnc", "attentionDec", "attentionDecCross",
	"selfBlockDec", "layerNorm", "mel", "melToConvInput", "embed", "vocabSoftMax", "softMaxSample", "eventPair", "layerNormDec", "gemmDecode" };
// "layerNormDec" / "gemmDecode" = the LayerNorm launches and the M-tiled products of the DECODER graph (prompt steps; the vocabulary product of more than
// 128 sequences): kept apart from the encoder's, whose classes are the MFMA roofline of the bench line

struct Profiler
{
	bool on = false;
	struct Pending { int kc; hipEvent_t a, b; };
	std::vector<Pending> pending;
	std::vector<hipEvent_t> pool;
	int64_t calls[ KC_COUNT ] = {};
	double ms[ KC_COUNT ] = {}, flops[ KC_COUNT ] = {}, bytes[ KC_COUNT ] = {};
	hipEvent_t get()
	{
		if( !pool.empty() ) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
		hipEvent_t e = nullptr;
		(void)hipEventCreate( &e );
		return e;
	}
	void resolve()
	{
		for( const Pending& p : pending )
		{
			float t = 0;
			if( hipEventSynchronize( p.b ) == hipSuccess && hipEventElapsedTime( &t, p.a, p.b ) == hipSuccess ) ms[ p.kc ] += t;
			pool.push_back( p.a );
			pool.push_back( p.b );
		}
		pending.clear();
	}
	void reset()
	{
		resolve();
		for( int i = 0; i < KC_COUNT; i++ ) { calls[ i ] = 0; ms[ i ] = flops[ i ] = bytes[ i ] = 0; }
	}
	~Profiler()
	{
		resolve();
		for( hipEvent_t e : pool ) (void)hipEventDestroy( e );
	}
};

// The per-layer hook of wh_align_tokens in the multi-token decoder graph: behind the cross-attention query of layers layer0 .. layer1 the rows are copied
// to q + ( layer - layer0 ) * layerStride, and the pass ends behind layer1's query (nothing later is read: no MLP, no vocabulary product).
struct AlignHook { int layer0, layer1; wh::f16* q; int64_t layerStride; };

// What a context holds of the decode-step logit filters (filters.hip, the only unit that names a member; the interface the other units use is further down).
// A switch per filter and its device buffers, each allocated by the first call that turns its filter on -- before any capture -- and never again: a captured step
// keeps the addresses and reads the values behind them, so a new set, boost or window recaptures nothing.
struct LogitFilters
{
	// wh_context_set_suppress: suppressSet = [ count ][ ids: eot ] int32, suppressHeld its count on the host; suppressOff: bypassFilterLogits
	int suppressHeld = 0;
	int* suppressSet = nullptr;
	bool suppressOff = false;
	// wh_context_set_timestamp_rules: ruleRecords [maxSeq]
	bool rulesOn = false;
	wh::TimestampRecord* ruleRecords = nullptr;
	// wh_context_set_boost: phraseTables [BOOST_TABLE_INTS], phraseStates [maxSeq]
	bool phrasesOn = false;
	int *phraseTables = nullptr, *phraseStates = nullptr;
	// wh_context_set_no_repeat: ngramN = n, 0 = off; ngramHistory [maxSeq][n_text_ctx], ngramCounts [maxSeq]
	int ngramN = 0;
	int *ngramHistory = nullptr, *ngramCounts = nullptr;
};

struct wh_context
{
	wh_model* m = nullptr;
	Profiler prof;
	int maxBatch = 0;	   // 30 s windows (encoder batch, cross-attention caches)
	int hyp = 1;		   // decoder hypotheses per window: rows b*hyp .. b*hyp+hyp-1 share window b's cross-attention K/V
	int maxSeq = 0;		   // decoder sequences = maxBatch * hyp (self-attention caches, logits, sampler state)
	hipStream_t stream = nullptr;
	uint32_t flags = 0;
	int parityThreads = 1;
	int T = 0, Tpad = 0, maxRows = 0;
	int64_t vram = 0;
	bool encoded = false;
	int lastBatch = 0;	   // decoder sequences of the last decode call
	int lastEncBatch = 0;  // windows of the last wh_encode
	int encChunk = 0;	   // windows the ENCODER runs at a time: its activations are sized for this many, a larger lock-step batch is encoded in
						   // equal chunks (the products are MFMA-bound and saturated at ~100 windows; only the cross-attention caches hold all windows)
	// encoder activations
	f16 *convIn = nullptr, *conv1Out = nullptr, *xn = nullptr, *q = nullptr, *k = nullptr, *vT = nullptr, *attn = nullptr, *h = nullptr;
	float* x = nullptr;
	int64_t convInStride = 0, conv1Stride = 0;
	// caches
	f16 *crossK = nullptr, *crossV = nullptr, *selfK = nullptr, *selfV = nullptr;
	// decoder activations
	float *dx = nullptr, *logits = nullptr, *probs = nullptr;
	f16 *dxn = nullptr, *dq = nullptr, *dattn = nullptr, *dh = nullptr;
	float* splitK = nullptr;	 // [8][min( maxRows, 128 )][d]: partial tiles of the K-split MLP down-projection (option dec_split)
	// single-stream decode steps (decode1.hip): cross-attention scores, per-split maxima and partial results of up to 4 sequences
	float *crossScores = nullptr, *crossSplitMax = nullptr, *crossPart = nullptr;
	int* tokensDev = nullptr;
	int* melOffsetsDev = nullptr;
	MelWindow* melWindowsDev = nullptr;
	TokenData* tokDataDev = nullptr;
	uint8_t* sampleScratch = nullptr;		   // TUNE_SAMPLE_SPREAD: slice records of the spread sampler (allocated on first use, before any capture)
	float* langP = nullptr;					   // wh_lang_detect: [maxBatch][n_lang] probabilities and [maxBatch] winners (allocated on first use)
	int* langBest = nullptr;
	// temperature sampling (wh_context_set_sampling): 0 = the greedy sampler. The factor, seed and nonce live in device memory (allocated by the first call with a
	// temperature above 0, before any capture), so one captured step graph per mode serves every attempt
	float temperature = 0.0f;
	SampleParams* sampleParams = nullptr;
	// per-row sampling (wh_context_set_sampling_rows): sampleRowsOn != 0 = every sequence samples under its own record of sampleRows [maxSeq] (device; allocated,
	// like its pinned staging and the event behind the staging's last upload, by the first call that turns the mode on, before any capture)
	int sampleRowsOn = 0;
	SampleRowParams *sampleRows = nullptr, *sampleRowsPin = nullptr;
	hipEvent_t sampleRowsEv = nullptr;
	LogitFilters filters;	   // the decode-step logit filters: filters.hip alone reads or writes a member
	// wh_context_set_no_speech: p[ solm ] of the prompt step's rows, gathered behind the first sample of every window (allocated by the first call that turns it on)
	bool noSpeech = false;
	float* noSpeechDev = nullptr;
	hipEvent_t noSpeechEv = nullptr;
	int noSpeechRows = 0;	   // rows the window in progress gathered (0 = none)
	// wh_align_tokens (align.hip; all allocated on first use, outside every captured graph): the query rows of the selected layers, the last call's matrix,
	// the softmax maxima and sums of sweep 1, the frames, and the call's head list and per-window sizes
	f16* alignQ = nullptr;
	float *alignM = nullptr, *alignStats = nullptr;
	int *alignFrames = nullptr, *alignMeta = nullptr;
	int alignBatch = 0, alignNMax = 0, alignLayer0 = 0, alignLayer1 = 0;	   // what the last call left for wh_debug_read
	const struct AlignHook* alignHook = nullptr;   // set around the pass of wh_align_tokens only
	// wh_score_tokens (align.hip; all allocated on first use, outside every captured graph): the gathered rows of the normalised activations, the logits of one
	// chunk of them, the targets and records of all of them, the call's per-window sizes
	f16* scoreRows = nullptr;
	float* scoreLogits = nullptr;
	TokenScore* scoreOut = nullptr;
	int *scoreTargets = nullptr, *scoreMeta = nullptr;
	bool scoreHook = false;	   // set around the pass of wh_score_tokens only: the multi-token decoder graph ends behind the final LayerNorm of all its rows
	// wh_context_speech_filter (speech.hip; all allocated by the first call that needs them, grown on demand, outside every captured graph): the features of
	// the recording's frames, the span table the pack kernel reads, and the packed copies of the mono and the stereo buffer
	float *speechFeat = nullptr, *speechMono = nullptr, *speechStereo = nullptr;
	long long* speechTable = nullptr;
	TokenData* beamCand = nullptr;			   // beam search: [maxSeq][8] candidates (allocated on first use)
	f16 *selfKScratch = nullptr, *selfVScratch = nullptr;	   // beam search: the copy a cache reorder goes through (allocated on first use)
	// beam search on the device (wh_beam_window_*): per-window rules and state, the records of every step, the parents a step's reorder reads
	BeamRules* beamRules = nullptr;
	BeamWindow* beamState = nullptr;
	BeamRecord* beamRecords = nullptr;
	int* beamParents = nullptr;
	int beamWindows = 0, beamWidth = 0, beamSteps = 0;	   // the window in progress: windows, width, ranking steps enqueued so far
	float* melScratch = nullptr;
	// device-side greedy loop: the sampler's state and one position per sequence (the sequences of a lock-step batch may differ)
	DecodeState* state = nullptr;
	int* seqPos = nullptr;
	// host mailbox of the greedy loop (pinned, coherent): [n_text_ctx * maxSeq] records + stamps, and the generation of the window in progress
	TokenData* mailData = nullptr;
	int* mailFlag = nullptr;
	SampleMailbox mailDev = { nullptr, nullptr };
	int mailGen = 0;		   // generation of the window in progress (0 = its samples are not mirrored)
	int mailCounter = 0;	   // last generation handed out
	TokenData* greedyOut = nullptr;	   // [n_text_ctx][maxBatch]
	// the captured decode steps of every kind, by ( batch, stepKey ): owned by step_graph.hip, which states the key and the retention rule. stepCaptures counts the
	// graphs instantiated over the context's life (wh_debug_step_captures)
	struct StepGraph { int batch; uint32_t key; hipGraphExec_t exec; };
	std::vector<StepGraph> stepGraphs;
	int stepCaptures = 0;
	hipGraphExec_t stepGraph( int batch, uint32_t key ) const
	{
		for( const StepGraph& g : stepGraphs )
			if( g.batch == batch && g.key == key ) return g.exec;
		return nullptr;
	}
	void destroyStepGraphs()
	{
		for( const StepGraph& g : stepGraphs ) (void)hipGraphExecDestroy( g.exec );
		stepGraphs.clear();
	}
	const int* raggedLastPos = nullptr;	   // set around the prompt step of a window whose prompts differ in length: device [batch], position of each sequence's last prompt token
	int windowSamples = 0;
	int windowPos = 0;		   // position the next greedy step feeds (prompt length + steps enqueued so far)
	hipStream_t copyStream = nullptr;
	// TUNE_SPLIT_STREAMS: the MFMA-bound encoder on its own low-priority stream, so that the latency-bound decode chains of
	// OTHER contexts (high-priority streams) get their workgroups dispatched first whenever CUs free up
	hipStream_t encStream = nullptr;
	hipEvent_t encReady = nullptr, encDone = nullptr;
	hipEvent_t encGateEv = nullptr;	   // TUNE_ENC_SERIAL: recorded behind this context's encoder; the next context's encoder waits for it
	int encCus = 0, totalCus = 0;	   // WH_ENC_CUS: CUs of the encoder stream's mask (0 = no spatial split)
	struct Mark { int endSample; hipEvent_t ev; };
	std::vector<Mark> marks;   // after each enqueued chunk of samples: an event wh_decode_window_fetch can wait for
	std::vector<hipEvent_t> markPool;
	// WH_FLAG_DEBUG_CAPTURE: copies of intermediates at the reference's Tracing probe points (WhisperContext.cpp:142-638)
	f16 *capTemp1 = nullptr, *capEncKqv = nullptr, *capDecKqvSelf = nullptr, *capDecKqvCross = nullptr;
	float* capLayer0In = nullptr;
	int capDecRows = 0;
	int profKeysHint = 1;	   // profiler only: keys a device-positioned self-attention launch sees (host mirror of the largest position + 1)
	// WH_FLAG_PARITY_EXACT (exact.hip): FP32 activations of the reference-order graph, allocated on first use for up to EXACT_CHUNK windows of n_audio_ctx
	// frames at a time (a larger batch is encoded chunk by chunk), the decoder's rows and score scratch grown on demand; ggml_init's two 65536-entry tables
	struct Exact
	{
		static constexpr int CHUNK = 8;
		f16 *gelu = nullptr, *expt = nullptr;
		float *x = nullptr, *cur = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *kqv = nullptr, *h = nullptr, *conv1 = nullptr;
		float *dx = nullptr, *dcur = nullptr, *dq = nullptr, *dk = nullptr, *dv = nullptr, *dkqv = nullptr, *dh = nullptr, *scores = nullptr;
		int encWindows = 0;
	} ex;
	bool ownsStream = false;
	// pinned host staging for fully asynchronous enqueues: ints [0, 4096) window offsets or descriptors (6 ints each: up to 682 windows),
	// [4096, 4104) the sampler state, [4104, 4104 + maxSeq) positions, then the prompt tokens of a window (up to n_text_ctx per sequence)
	int32_t* pinned = nullptr;
	int64_t pinnedInts = 0;
	static constexpr int PIN_WINDOWS = 4096, PIN_STATE = PIN_WINDOWS, PIN_POS = PIN_STATE + 8;
	int32_t* pinTokens() const { return pinned + PIN_POS + maxSeq; }
	int64_t pinTokenCap() const { return pinnedInts - PIN_POS - maxSeq; }
	// The ONE owner of the context's device memory: every buffer is in `allocations` and counted in `vram`, wh_context_destroy verifies and frees them all.
	std::vector<Allocation> allocations;

	// Every buffer starts zeroed. MUST_BE_ZERO marks the ones whose correctness depends on it: the convolution padding
	// rows, the V operand padding, the K/V caches (rows beyond n_past are masked, not skipped: they must be finite) and the
	// device-resident decode state. The others are written before they are read and are zeroed only as hygiene -- which is
	// exactly what WH_DEBUG_POISON=<byte> checks: in that mode those buffers are filled with the byte instead (0xFF = NaN in
	// FP16 / FP32 and -1 as an index), every buffer gets a guard region on both sides, and wh_context_destroy verifies the
	// guards. A run whose results or faults change under WH_DEBUG_POISON depends on stale device memory.
	enum eInit { DONT_CARE, MUST_BE_ZERO };
	template<class T> int alloc( T*& p, int64_t count, eInit init, const char* name )
	{
		Allocation a;
		WH_HIP( guardedAlloc( a, count * (int64_t)sizeof( T ), ( init == DONT_CARE && debugPoison() >= 0 ) ? debugPoison() : 0, name, stream ) );
		allocations.push_back( a );
		vram += a.bytes;
		p = (T*)a.body;
		return 0;
	}
	// Gives one buffer back: guards verified, hipFree, out of `allocations` and `vram`. The caller has waited for whatever used it.
	template<class T> void release( T*& p )
	{
		for( size_t i = 0; i < allocations.size(); i++ )
			if( allocations[ i ].body == (void*)p )
			{
				vram -= allocations[ i ].bytes;
				(void)guardedFree( allocations[ i ] );
				allocations.erase( allocations.begin() + (ptrdiff_t)i );
				break;
			}
		p = nullptr;
	}
	// Grow on demand: nothing when p already holds `count` elements. Otherwise the stream is waited for, the old buffer released (its CONTENT IS
	// LOST) and a new one allocated, of at least twice the old size so that a buffer that grows step by step is not reallocated every step.
	// A captured graph keeps the addresses it was captured with, so a buffer must never be released while such a graph is alive: only paths that
	// are never captured call this -- exact mode, and the first-use allocations that happen before any capture.
	template<class T> int grow( T*& p, int64_t count, eInit init, const char* name )
	{
		int64_t have = 0;
		if( p )
			for( const Allocation& a : allocations )
				if( a.body == (void*)p ) have = a.bytes / (int64_t)sizeof( T );
		if( count <= have ) return 0;
		if( p )
		{
			WH_HIP( hipStreamSynchronize( stream ) );
			release( p );
		}
		return alloc( p, count > 2 * have ? count : 2 * have, init, name );
	}
	static constexpr int GUARD_BYTE = 0xA5;
	static int debugPoison()
	{
		static const int v = []() { const char* e = getenv( "WH_DEBUG_POISON" ); return ( e && *e ) ? (int)( strtol( e, nullptr, 0 ) & 0xFF ) : -1; }();
		return v;
	}
	static int64_t debugGuardBytes() { return debugPoison() >= 0 ? 65536 : 0; }
};


// Debug capture: device-to-device copy of an intermediate into a lazily allocated side buffer (stream-ordered).
template<class T>
static int capture( wh_context* c, T*& dst, const T* src, int64_t count, int64_t capacity )
{
	if( !( c->flags & WH_FLAG_DEBUG_CAPTURE ) ) return 0;
	if( !dst ) WH_CHECK( c->alloc( dst, capacity, wh_context::DONT_CARE, "debug capture" ) );
	WH_HIP( hipMemcpyAsync( dst, src, (size_t)count * sizeof( T ), hipMemcpyDeviceToDevice, c->stream ) );
	return 0;
}

// WH_DEBUG_SYNC=1: every launch is announced on stderr and waited for (and nothing is captured into a hipGraph), so that a
// device fault can be attributed to a kernel class from the log of a dead process.
inline bool debugSync()
{
	static const bool v = []() { const char* e = getenv( "WH_DEBUG_SYNC" ); return e && *e && *e != '0'; }();
	return v;
}

// Runs one launch, optionally bracketed by events. flops / bytes are the ALGORITHMIC work of the launch.
template<class F>
static int profiled( wh_context* c, int kc, double flops, double bytes, F&& launch )
{
	Profiler& p = c->prof;
	if( debugSync() )
	{
		// breadcrumbs: a `Memory access fault by GPU` kills the process, the last line on stderr then names the launch
		fprintf( stderr, "[wh] launch %s\n", kernelClassNames[ kc ] );
		fflush( stderr );
		const int rc = launch();
		const hipError_t e = hipStreamSynchronize( c->stream );
		if( e != hipSuccess ) return hipFail( e, kernelClassNames[ kc ], __FILE__, __LINE__ );
		return rc;
	}
	if( !p.on ) return launch();
	hipEvent_t a = p.get(), b = p.get();
	WH_HIP( hipEventRecord( a, c->stream ) );
	const int rc = launch();
	WH_HIP( hipEventRecord( b, c->stream ) );
	p.pending.push_back( { kc, a, b } );
	p.calls[ kc ]++;
	p.flops[ kc ] += flops;
	p.bytes[ kc ] += bytes;
	if( p.pending.size() >= 4096 ) p.resolve();
	return rc;
}
// contexts alive PER DEVICE: a model on another adapter of the same process is nobody's neighbour
namespace wh { extern std::atomic<int> g_liveContextsDev[ 64 ]; }
inline std::atomic<int>& liveContexts( const wh_model* m ) { return g_liveContextsDev[ m->device & 63 ]; }
// TUNE_ENC_SERIAL: the encoders of the contexts of one device form a chain -- an encoder starts when the previous one (of another
// context) has finished. Stream-ordered (hipStreamWaitEvent), the host never blocks. Two batches started together then run out of
// phase from the first round on: while one decodes (launch latencies, HBM), the other's encoder has the matrix cores.
namespace wh
{
	extern std::mutex g_encGateMx;
	struct EncGate { hipEvent_t last = nullptr; const wh_context* owner = nullptr; };
	extern EncGate g_encGate[ 64 ];
	constexpr int ENC_SERIAL_MIN_WINDOWS = 8;	  // a one-window context (a single stream, a loader) neither waits nor makes others wait

	// helpers more than one unit needs
	int gemmP( wh_context* c, const GemmArgs& g, bool skinny, bool decoder = false );
	int lnP( wh_context* c, const float* x, const float* w, const float* b, f16* out, int rows, int d, bool decoder = false );
	GemmArgs plainGemm( const f16* A, const f16* W, int M, int N, int K );
	int exactTables( wh_context* c );
	int encodeExact( wh_context* c, const float* melDev, int batch, int64_t melLen, int64_t melStride, const int32_t* melOffsets, const wh_mel_window* wins );
	int decodeExact( wh_context* c, int batch, int nTokens, int nPast );
	int decodeGraph( wh_context* c, int batch, int nTokens, int nPast, bool devState );
	int checkTokens( const wh_hparams& hp, const int32_t* tokens, int64_t count, const char* who );
	int uploadDecodeState( wh_context* c, int batch, const DecodeState& s, const int32_t* positions, int uniform );
	int alignDebugRead( wh_context* c, const std::string& w, int layer, float* dstHost, int64_t dstCapFloats );

	// captured decode steps (step_graph.hip, where each of these is explained)
	constexpr uint32_t STEP_KEY_ROWS = 0x40000u, STEP_KEY_BEAM = 0x200000u;	  // bits 19, 20 and 26-30 are the filters' (filterGraphKey, filterLoopKey)
	using StepFn = std::function<int()>;
	enum eWarmUp { WARM_FRESH, WARM_PRESERVE };
	bool stepsReplayable( const wh_context* c );
	uint32_t stepKey( const wh_context* c, int beamWidth );	   // beamWidth 0: a step of the greedy loop
	int obtainStepGraph( wh_context* c, int batch, uint32_t key, eWarmUp warm, const StepFn& idle, const StepFn& step, hipGraphExec_t& exec );
	int idleLoopState( wh_context* c, int batch );
	int enqueueSteps( wh_context* c, hipGraphExec_t exec, int nSteps, int firstKeys, const StepFn& step );
	// what WARM_PRESERVE carries over the warm-up step: the list is stated next to the step that mutates it (decode.hip); `filters` is saveFilterState's
	struct LoopState { DecodeState state; std::vector<int32_t> pos, tok; std::vector<uint8_t> filters; };
	int saveLoopState( wh_context* c, int batch, LoopState& s );
	int restoreLoopState( wh_context* c, int batch, const LoopState& s );

	// the decode-step logit filters (filters.hip, where each of these is explained): all that the other units know of them
	enum eFilterPhase { FILTER_STEP = 0, FILTER_WINDOW = 1, FILTER_ARM = 2 };	  // a step of the loop; behind a window's prompt step; wh_decode_greedy, whose first token is no sample
	int filterLogits( wh_context* c, int batch );							  // the end of decodeGraph
	void bypassFilterLogits( wh_context* c, bool on );						  // around wh_lang_detect's pass
	int filterLoopRows( wh_context* c, int batch, eFilterPhase phase );	  // between decodeGraph and the sampler of the device-side loop
	uint32_t filterGraphKey( const wh_context* c );							  // stepKey's bits of every step that runs decodeGraph
	uint32_t filterLoopKey( const wh_context* c );							  // ... and of a step of the greedy loop
	int saveFilterState( const wh_context* c, int batch, std::vector<uint8_t>& s );
	int restoreFilterState( wh_context* c, int batch, const std::vector<uint8_t>& s );
	int filtersAllowFlags( const wh_context* c, uint32_t flags );			  // wh_context_set_flags: 0, or the refusal with its error set
}

static inline uint16_t f32ToF16Bits( float f )
{
	const _Float16 h = (_Float16)f;
	uint16_t u;
	memcpy( &u, &h, 2 );
	return u;
}
static inline float f16BitsToF32( uint16_t u )
{
	_Float16 h;
	memcpy( &h, &u, 2 );
	return (float)h;
}
