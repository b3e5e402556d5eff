/* whisper_c.h -- flat C mirror of the COM-style API in whisperApi.h, exported by libWhisper.so for FFI callers that cannot
 * consume C++ vtables (Python ctypes, cgo, JNI, N-API). Every function forwards to the iModel / iContext method named in
 * its comment (reference: Whisper/API/iContext.cl.h:23-60); return values are the HRESULTs of those methods.
 * Opaque handles are COM object pointers: release each with whisperc_release. */
#ifndef WHISPER_C_H
#define WHISPER_C_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* Whisper::loadModel( path, { GPU, adapter = device }, nullptr, &model ) */
int32_t whisperc_load_model( const char* pathUtf8, int device, void** modelOut );
/* IUnknown::Release */
void whisperc_release( void* unknown );
/* iModel::createContext */
int32_t whisperc_create_context( void* model, void** ctxOut );
/* iModel::getSpecialTokens -> { eot, sot, prev, solm, not, beg, translate, transcribe } */
int32_t whisperc_special_tokens( void* model, int32_t* out8 );
/* iModel::stringFromToken (pointer into the model's vocabulary, valid while the model lives) */
const char* whisperc_token_string( void* model, int token );
/* iModel::isMultilingual: S_OK (0) or S_FALSE (1) */
int32_t whisperc_is_multilingual( void* model );
/* iModel::tokenize: returns the token count (>= 0) or a failed HRESULT */
int32_t whisperc_tokenize( void* model, const char* text, int32_t* out, int cap );
/* iContext::fullDefaultParams( Greedy ) + the given fields, then iContext::runFull on a mono FP32 16 kHz buffer.
 * flags = eFullParamsFlags bits (Translate 1, NoContext 2, SingleSegment 4, PrintSpecial 8 ...). */
int32_t whisperc_run_full( void* ctx, const float* pcm, uint32_t nSamples, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx /* < 0 keeps the default 16384 */ );
/* The same with eSamplingStrategy::BeamSearch and beam_search.beam_width = beamWidth (1 .. 8; the reference declares the strategy,
 * Whisper/API/sFullParams.h:10-13, and implements only Greedy): beamWidth hypotheses per window share one pass over its cross-attention K/V. */
/* whisperc_run_full + sFullParams::offset_ms / duration_ms (0 = to the end): the range of the buffer that is transcribed */
int32_t whisperc_run_full_range( void* ctx, const float* pcm, uint32_t nSamples, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, int offsetMs, int durationMs );
/* whisperc_run_full + sFullParams::audio_ctx (encoder positions / cross-attention keys per window; 0 = the model's) */
int32_t whisperc_run_full_audio_ctx( void* ctx, const float* pcm, uint32_t nSamples, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, int audioCtx );
int32_t whisperc_run_full_beam( void* ctx, const float* pcm, uint32_t nSamples, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, int beamWidth );
/* iMediaFoundation::loadAudioFileData( WAV bytes: PCM of 8 .. 32 bits or float32, 1 .. 8 channels, any rate from 1 to 384 kHz ) + iContext::runStreamed( params,
 * { progress callback }, reader ): the streaming entry the reference's CLI uses by default (Examples/main/main.cpp:305-311).
 * The values the progress sink received are copied to progressOut (first progressCap of them), their count to *progressCount. */
int32_t whisperc_run_streamed( void* ctx, const void* wavBytes, uint64_t wavSize, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, double* progressOut, int progressCap, int* progressCount );
/* Audio of any rate -> 16 kHz FP32 on the GPU (wh_resample_host of whisper_hip.h, on the calling thread's current device): nFrames interleaved frames of
 * `channels` samples in `format` (0 u8, 1 s16, 2 s24, 3 s32, 4 float32) at `rate` Hz; channel -1 = the mean of the channels, else that channel.
 * *nOut = ceil( nFrames * 16000 / rate ); dst == NULL only counts, cap (floats of dst) < *nOut is E_INVALIDARG. rate 16000 converts without filtering. */
int32_t whisperc_resample( const void* src, int32_t format, int32_t channels, int32_t channel, int32_t rate, int64_t nFrames, float* dst, int64_t cap,
	int64_t* nOut );
/* Live transcription (Whisper::createPcmCapture, iPcmCapture, iContext::runCapture of whisperApi.h): a capture is a queue of PCM chunks -- at 16 kHz, or at sampleRate with whisperc_capture_create_rate -- that the caller
 * writes from any thread -- format 1 = s16, 4 = float32; 1 or 2 interleaved channels, the same in every call -- and whisperc_run_capture drains on another:
 * the reference's capture loop (voice activity per chunk on the GPU; a piece is fired at a pause once minDuration is buffered, or at maxDuration) with every
 * piece transcribed by iContext::runFull on a worker thread, segment times being stream times. Durations in seconds (the reference's defaults are 2, 3, 0.25,
 * 0.333); flags: 1 = keep stereo (whisperc_result_speakers then answers per piece), 2 = NoDrop: never discard samples, wait for the running transcription
 * instead (a source that is not real time; whisperc_capture_write then blocks while more than maxDuration + 1 s is queued and a loop is draining).
 * whisperc_capture_close marks the end of the stream: the loop drains the queue, transcribes what is left if it holds voice and returns 0.
 * whisperc_run_capture: language and flags as whisperc_run_full. pfnShouldCancel is asked before every read, anything but 0 ends the call with 0;
 * pfnCaptureStatus receives the status word (Listening 1, Voice 2, Transcribing 4, Stalled 0x80) whenever a bit changes -- on the calling thread, but for the fall of Transcribing without NoDrop, which
 * comes from the worker thread when the piece's transcription ends, as in the reference;
 * pfnPiece( pv, startSample, nSamples ) is called behind each piece's transcription, on the library's worker thread, while whisperc_result_* answer for
 * that piece. Each may be NULL. E_POINTER for a NULL capture, E_INVALIDARG for minDuration or maxDuration outside [0.125, 30]. */
int32_t whisperc_capture_create( float minDuration, float maxDuration, float dropStartSilence, float pauseDuration, uint32_t flags, void** captureOut );
/* Whisper::createPcmCaptureAtRate: what is written has sampleRate frames per second, 1000 .. 384000 or E_INVALIDARG, and is resampled to 16 kHz on the device chunk
 * by chunk; durations, start samples and times stay those of the 16 kHz stream. 16000 is whisperc_capture_create. */
int32_t whisperc_capture_create_rate( float minDuration, float maxDuration, float dropStartSilence, float pauseDuration, uint32_t flags, uint32_t sampleRate,
	void** captureOut );
int32_t whisperc_capture_write( void* capture, const void* samples, int32_t format, int32_t channels, uint32_t frames );
int32_t whisperc_capture_close( void* capture );
/* chunks dropped by whisperc_capture_write because the loop did not keep up (never under NoDrop) */
uint64_t whisperc_capture_dropped( void* capture );
void whisperc_capture_destroy( void* capture );
int32_t whisperc_run_capture( void* ctx, void* capture, const char* language, uint32_t flags, int32_t ( *pfnShouldCancel )( void* pv ),
	int32_t ( *pfnCaptureStatus )( void* pv, uint8_t status ), void ( *pfnPiece )( void* pv, int64_t startSample, int64_t nSamples ), void* pv );
/* The same with the further parameters of whisperc_run_full / _audio_ctx / _beam, which then hold for every piece: maxTokens, the prompt, nMaxTextCtx (< 0 keeps
 * the default), audioCtx (0 = the model's), beamWidth (0 = greedy). */
int32_t whisperc_run_capture_params( void* ctx, void* capture, const char* language, uint32_t flags, int maxTokens, const int32_t* promptTokens, int nPrompt,
	int nMaxTextCtx, int audioCtx, int beamWidth, int32_t ( *pfnShouldCancel )( void* pv ), int32_t ( *pfnCaptureStatus )( void* pv, uint8_t status ),
	void ( *pfnPiece )( void* pv, int64_t startSample, int64_t nSamples ), void* pv );
/* Splitting a long recording at pauses (Whisper::splitAtPauses of whisperApi.h), on mono FP32 16 kHz PCM:
 * whisperc_vad: voice-activity features on the calling thread's current device (wh_vad_features_host of whisper_hip.h), then the reference's decision loop
 *   (Whisper/Whisper/voiceActivityDetection.cpp:121-205) on the host: speech[ f ] = 1 where frame f = samples [256 f, 256 f + 256) is speech, *lastSpeech =
 *   ( f + 1 ) * 256 of the last speech frame (0 = none), *nFrames = nSamples / 256. speech == NULL only counts; cap < *nFrames is E_INVALIDARG.
 * whisperc_plan_chunks: the chunks (first[ i ], count[ i ]) in samples that partition the recording into pieces of at most maxLen and -- but for the last --
 *   at least minLen samples, cut in the middle of pauses of at least pauseFrames frames, or where 21 frames hold the least energy when there is no pause
 *   (whisper_amd/host/chunkPlanner.h states the rule). 0 = the defaults 480000 / 240000 / 21; 16000 <= minLen <= maxLen - 32000, maxLen <= 480000, or
 *   E_INVALIDARG. *nChunks = the chunks; first / count may be NULL (count only), cap < *nChunks is E_INVALIDARG.
 * whisperc_debug_vad_decide: the host half on its own (no device): the decision loop over nFrames x ( energy, F, SFM ); speech may be NULL. */
int32_t whisperc_vad( const float* pcm, int64_t nSamples, uint8_t* speech, int64_t cap, int64_t* nFrames, int64_t* lastSpeech );
int32_t whisperc_plan_chunks( const float* pcm, int64_t nSamples, int64_t maxLen, int64_t minLen, int32_t pauseFrames, int64_t* first, int64_t* count,
	int32_t cap, int32_t* nChunks );
int32_t whisperc_debug_vad_decide( const float* feat, int64_t nFrames, uint8_t* speech, int64_t* lastSpeech );
/* iMediaFoundation::loadAudioFile + iAudioBuffer::getPcmMono (stereo != 0: getPcmStereo, interleaved, 2 floats per frame; a mono file, whose buffer has no stereo data, twice): the WAV file as 16 kHz floats.
 * *nFrames = its 16 kHz frames; dst == NULL reads the file and parses its chunks, converts nothing and returns the count (so a
 * caller that asks for the count first reads the file twice); cap counts floats. */
int32_t whisperc_load_audio( const char* pathUtf8, int32_t stereo, float* dst, int64_t cap, int64_t* nFrames );
/* whisperc_run_full + the token-timestamp fields of sFullParams (set TokenTimestamps = 0x100 in flags): thold_pt, thold_ptsum, max_len */
int32_t whisperc_run_full_tt( void* ctx, const float* pcm, uint32_t nSamples, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, float tholdPt, float tholdPtsum, int maxLen );
/* Whisper::setAlignmentHeads: the (layer, head) pairs whose cross-attention weights the AlignTokens flag (0x1000 in flags: token times by dynamic time
 * warping; through whisperc_run_full, _range, _audio_ctx, _tt for max_len, and whisperc_run_streamed) averages; count 0 restores the default heads */
int32_t whisperc_model_set_alignment_heads( void* model, const int32_t* layerHeadPairs, int32_t count );
/* Whisper::setDecodingFallback on an iContext: on != 0 turns the temperature fallback and the quality gates on with these sDecodingFallback values (the
 * defaults are 0.2, -1, 2.4, 0.6 and seed 0), on == 0 turns them off, the state of every new context; then a run's transcript is what it always was.
 * whisperc_window_stats: Whisper::getWindowStats, what the fallback did with each window of the context's last run. out = sWindowStats [cap] of whisperApi.h
 * { int32 seek, attempts; float temperature, noSpeech; double avgLogprob, entropy; uint32 skipped, reserved } or NULL, *count = the number of windows;
 * cap smaller than that with a non-NULL out is E_BOUNDS. */
int32_t whisperc_set_fallback( void* ctx, int32_t on, float temperatureInc, float logprobThold, float entropyThold, float noSpeechThold, uint64_t seed );
int32_t whisperc_window_stats( void* ctx, void* out, uint32_t cap, uint32_t* count );
/* The same for a batch runner (Whisper::setBatchDecodingFallback): every later run of the runner; a window whose attempt fails is decoded again in its slot in
 * the group's next round (one slot-round per retry), stream i draws under the key seed + i. whisperc_tr_window_stats: Whisper::getResultWindowStats, the
 * windows of the stream a result object of whisperc_batch_run belongs to; out / cap / count as whisperc_window_stats. */
int32_t whisperc_batch_set_fallback( void* runner, int32_t on, float temperatureInc, float logprobThold, float entropyThold, float noSpeechThold, uint64_t seed );
int32_t whisperc_tr_window_stats( void* result, void* out, uint32_t cap, uint32_t* count );
/* Suppressed tokens (Whisper::getNonSpeechTokens / setSuppressedTokens / setBatchSuppressedTokens of whisperApi.h): the logits of the given text-token ids
 * (each in [0, eot)) are -inf before the softmax in every later run. whisperc_non_speech_tokens: the model's non-speech set, ascending; out = int32 [cap] or
 * NULL, *count = its size; cap smaller than that with a non-NULL out is E_BOUNDS. count == 0 (ids may be NULL) turns suppression off, the state of every new
 * context and runner. */
int32_t whisperc_non_speech_tokens( void* model, int32_t* out, uint32_t cap, uint32_t* count );
int32_t whisperc_set_suppress_tokens( void* ctx, const int32_t* ids, uint32_t count );
int32_t whisperc_batch_set_suppress_tokens( void* runner, const int32_t* ids, uint32_t count );
/* Phrase boosting (Whisper::setBoostedPhrases / setBatchBoostedPhrases / phraseSpellings of whisperApi.h): tokens = int32 [count][nMax], row p holds lens[ p ]
 * text-token ids; boost is added to the logits of the tokens that continue a phrase. count == 0 turns it off (the pointers may be NULL), the state of every new
 * context and runner. whisperc_phrase_spellings: tokens = int32 [cap][16], lens = int32 [cap], *count = the rows written (1 or 2). */
int32_t whisperc_set_boost_phrases( void* ctx, const int32_t* tokens, const int32_t* lens, uint32_t count, uint32_t nMax, float boost );
int32_t whisperc_batch_set_boost_phrases( void* runner, const int32_t* tokens, const int32_t* lens, uint32_t count, uint32_t nMax, float boost );
int32_t whisperc_phrase_spellings( void* model, const char* text, int32_t* tokens, int32_t* lens, uint32_t cap, uint32_t* count );
/* No-repeat n-grams (Whisper::setNoRepeatNgram / setBatchNoRepeatNgram of whisperApi.h): n = 1 .. 8 = every later run forbids a text token that would complete an
 * n-gram its window has already sampled; 0 = off, the state of every new context and runner. */
int32_t whisperc_set_no_repeat_ngram( void* ctx, int32_t n );
int32_t whisperc_batch_set_no_repeat_ngram( void* runner, int32_t n );
/* Speech only (Whisper::setSpeechFilter / setBatchSpeechFilter / speechSpans / getSpeechSpans / getResultSpeechSpans of whisperApi.h): on != 0 = every later run
 * finds the speech with the voice-activity detector, transcribes only that and reports times on the recording's clock. Parameters in frames of 256 samples,
 * 0 = the defaults 125 / 16 / 25; negative or above 2^20 is E_INVALIDARG. on == 0 is the state of every new context and runner.
 * whisperc_speech_spans: the spans alone for a bare 16 kHz mono buffer, features on the calling thread's current device. whisperc_result_speech_spans: the spans
 * the context's last run used; whisperc_tr_speech_spans: those of the stream a result object of whisperc_batch_run belongs to, relative to the stream's first
 * sample. spans / out = int64 [cap][2] = first sample, end sample, or NULL; *count = the number of spans; cap smaller than that with a non-NULL buffer is E_BOUNDS. */
int32_t whisperc_set_speech_filter( void* ctx, int32_t on, int32_t minSilenceFrames, int32_t minSpeechFrames, int32_t padFrames );
int32_t whisperc_batch_set_speech_filter( void* runner, int32_t on, int32_t minSilenceFrames, int32_t minSpeechFrames, int32_t padFrames );
int32_t whisperc_speech_spans( const float* pcm, int64_t nSamples, int32_t minSilenceFrames, int32_t minSpeechFrames, int32_t padFrames, int64_t* spans,
	uint32_t cap, uint32_t* count );
int32_t whisperc_result_speech_spans( void* ctx, int64_t* out, uint32_t cap, uint32_t* count );
int32_t whisperc_tr_speech_spans( void* result, int64_t* out, uint32_t cap, uint32_t* count );
/* Timestamp rules (Whisper::setTimestampRules / setBatchTimestampRules of whisperApi.h): on != 0 = every later run masks the logits so that timestamps come in
 * pairs, never go back in time and close segments of non-zero length. Off is the state of every new context and runner. */
int32_t whisperc_set_timestamp_rules( void* ctx, int32_t on );
int32_t whisperc_batch_set_timestamp_rules( void* runner, int32_t on );
/* iContext::getResults( Tokens | Timestamps ) + iTranscribeResult::getSize / getSegments / getTokens; times in 100 ns ticks */
int32_t whisperc_result_counts( void* ctx, uint32_t* segments, uint32_t* tokens );
int32_t whisperc_result_segment( void* ctx, uint32_t index, uint64_t* t0, uint64_t* t1, uint32_t* firstToken, uint32_t* countTokens,
	char* text, uint32_t textCap );
int32_t whisperc_result_token( void* ctx, uint32_t index, int32_t* id, float* p, float* pt, float* ptsum );
/* sToken::time (100 ns ticks; 0 when unknown) and sToken::vlen of token `index` */
int32_t whisperc_result_token_times( void* ctx, uint32_t index, uint64_t* t0, uint64_t* t1, float* vlen );
/* Whisper::createBatchRunner( model, { maxSlots, groups, greedyChunk, flags } ) (0 = the defaults) -> iBatchRunner; release with whisperc_release */
int32_t whisperc_batch_create( void* model, uint32_t maxSlots, uint32_t groups, uint32_t greedyChunk, uint32_t flags, void** runnerOut );
/* iBatchRunner::run over `count` streams: stream i = samples [firstSample[i], firstSample[i] + countSamples[i]) (0 = to the end) of the mono FP32
 * 16 kHz buffer pcm[i] of nSamples[i] samples (streams may name the same buffer: the chunks of one recording); the common sFullParams are
 * fullDefaultParams( Greedy ) + the given fields, like whisperc_run_full. resultsOut[i] receives an iTranscribeResult (or NULL; release each with
 * whisperc_release), perStream[i] the stream's own HRESULT; both HOST arrays of `count` entries, perStream may be NULL. */
int32_t whisperc_batch_run( void* runner, uint32_t count, const float* const* pcm, const uint32_t* nSamples, const int64_t* firstSample,
	const int64_t* countSamples, const char* language, uint32_t flags, int maxTokens, const int32_t* promptTokens, int nPrompt, int nMaxTextCtx,
	void** resultsOut, int32_t* perStream );
/* Stereo diarization (iContext::detectSpeaker; the reference's rule, Whisper/Whisper/ContextImpl.diarize.cpp: the sum of |sample| per channel over the
 * segment, left if L > 1.1 R, right if R > 1.1 L, else unsure). `stereo` = nSamples interleaved frames (2 floats each, 16 kHz) of the recording whose mono
 * mix is `pcm`, what iAudioBuffer::getPcmStereo returns; NULL = no stereo data.
 * whisperc_run_full_stereo: whisperc_run_full_range over such a buffer.  whisperc_run_streamed_stereo: iContext::runStreamed over a reader of such PCM
 *   (progress as in whisperc_run_streamed).  whisperc_batch_run_stereo: whisperc_batch_run with stereo[i] beside pcm[i] (entries and the array may be NULL).
 * whisperc_detect_speaker: iContext::detectSpeaker( { t0, t1 } in 100 ns ticks ) -> *channel = eSpeakerChannel (0 unsure, 1 left, 2 right, 0xFF no stereo
 *   data). Like the reference's it answers only from the callbacks of a run; anywhere else OLE_E_BLANK (0x80040007).
 * whisperc_result_speakers / whisperc_tr_speakers: for callers without callbacks -- of a context's results / of a result object (a batch runner's
 *   per-stream result), one eSpeakerChannel byte per segment: what detectSpeaker answered for the segment's times when the segment was appended;
 *   0xFF = the run's audio had no stereo data. *count = the segments; out may be NULL (count only), cap < *count is E_INVALIDARG. */
int32_t whisperc_run_full_stereo( void* ctx, const float* pcm, const float* stereo, uint32_t nSamples, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, int offsetMs, int durationMs );
int32_t whisperc_run_streamed_stereo( void* ctx, const float* pcm, const float* stereo, uint32_t nSamples, const char* language, uint32_t flags, int maxTokens,
	const int32_t* promptTokens, int nPrompt, int nMaxTextCtx, double* progressOut, int progressCap, int* progressCount );
int32_t whisperc_batch_run_stereo( void* runner, uint32_t count, const float* const* pcm, const float* const* stereo, const uint32_t* nSamples,
	const int64_t* firstSample, const int64_t* countSamples, const char* language, uint32_t flags, int maxTokens, const int32_t* promptTokens, int nPrompt,
	int nMaxTextCtx, void** resultsOut, int32_t* perStream );
int32_t whisperc_detect_speaker( void* ctx, uint64_t t0, uint64_t t1, uint8_t* channel );
int32_t whisperc_result_speakers( void* ctx, uint8_t* out, uint32_t cap, uint32_t* count );
int32_t whisperc_tr_speakers( void* result, uint8_t* out, uint32_t cap, uint32_t* count );
/* iTranscribeResult::getSize / getSegments / getTokens on a result object itself (times in 100 ns ticks) */
int32_t whisperc_tr_counts( void* result, uint32_t* segments, uint32_t* tokens );
int32_t whisperc_tr_segment( void* result, uint32_t index, uint64_t* t0, uint64_t* t1, uint32_t* firstToken, uint32_t* countTokens, char* text, uint32_t textCap );
int32_t whisperc_tr_token( void* result, uint32_t index, int32_t* id, float* p, float* pt, float* ptsum, uint64_t* t0, uint64_t* t1, float* vlen );
/* Language detection (language "auto" / NULL / "" in the run entry points above: the language of every recording is detected on its first 30 s
 * window, frame 0 whatever the run's offset, and the run continues with it).
 * whisperc_detect_language: whisper_lang_auto_detect of the reference's CPU model (Whisper/source/whisper.cpp:2428-2495) on a mono FP32 16 kHz
 *   buffer: the window at offsetMs, probs[ id ] for the first probsCap language ids (99 languages; may be NULL), *langId = the winner.
 *   NOTE the reference's probs are a SECOND softmax over the language tokens' probabilities (exp( p ) / sum exp( p ) over numbers in [0, 1]):
 *   a clear winner comes back as ~0.02, not ~0.9. Offset before the start / past the end, or a model that is not multilingual: E_INVALIDARG.
 * whisperc_detected_language: what the last run (or whisperc_detect_language) on this context detected -- its code ("en", up to 4 characters + NUL)
 *   and its probs entry; S_FALSE (1) when nothing was detected (a named language, an .en model, less than a second of audio).
 * whisperc_debug_lang_probs: the host half on its own (no device): probs[ n ] from the n language-token probabilities p; returns the winner. */
int32_t whisperc_detect_language( void* ctx, const float* pcm, uint32_t nSamples, int32_t offsetMs, float* probs, uint32_t probsCap, int32_t* langId );
int32_t whisperc_detected_language( void* ctx, char* code5, float* p );
int32_t whisperc_debug_lang_probs( const float* p, int32_t n, float* probs );
/* Of a batch runner's per-stream result (whisperc_batch_run with language "auto": every stream gets ITS OWN language): the code and lang_probs entry
 * of the language the stream was detected and transcribed in; S_FALSE when the language was named. */
int32_t whisperc_tr_language( void* result, char* code5, float* p );
/* wh_context_set_flags( flags, parityThreads ) of include/whisper_hip.h on the device context behind this iContext, for parity tests: with
 * WH_FLAG_PARITY_EXACT (8) whisperc_detect_language returns the reference's lang_probs bit for bit. This context only. */
int32_t whisperc_debug_context_flags( void* ctx, uint32_t flags, int32_t parityThreads );
/* The code of language id (0 .. 98; the language token is sot + 1 + id) -> code5; S_FALSE beyond the table */
int32_t whisperc_language_code( int32_t id, char* code5 );
/* Scoring a given transcript (Whisper::scoreTokens / scoreBatch / makeSotSequence of whisperApi.h): teacher-forced token log-probabilities.
 * whisperc_sot_sequence: the tokens that select the task -- sot[, language, transcribe | translate], then the no-timestamps token unless `timestamps` -- into
 *   out[ cap ]; *count = their number (out may be NULL to ask for it; E_BOUNDS when cap is too small).
 * whisperc_score_tokens: the whole mono FP32 16 kHz buffer is the clip (1 to 30 s, one window); `prompt` is fed, `tokens` are scored and eot behind them:
 *   scoresOut receives count + 1 records of 32 bytes = { float logprob, bestLogprob; int32 best, rank; uint64 t0, t1 } (100 ns ticks; zero unless flags & 1 =
 *   forced alignment, which needs the no-timestamps token as the prompt's last entry and text tokens only).
 * whisperc_batch_score: `count` requests on a batch runner, up to its maxSlots per pass in request order; request i = samples [firstSample[i], firstSample[i] +
 *   countSamples[i]) (0 = to the end; the arrays may be NULL) of pcm[i], prompts[i] / tokens[i] with promptCounts[i] / counts[i] entries; scoresOut[i] receives
 *   counts[i] + 1 records, perRequest[i] (may be NULL) the request's own HRESULT. Returns the first failure. flags & 1 is E_NOTIMPL here. */
int32_t whisperc_sot_sequence( void* model, const char* language, int32_t translate, int32_t timestamps, int32_t* out, uint32_t cap, uint32_t* count );
int32_t whisperc_score_tokens( void* ctx, const float* pcm, uint32_t nSamples, const int32_t* prompt, uint32_t promptCount, const int32_t* tokens, uint32_t count,
	uint32_t flags, void* scoresOut );
int32_t whisperc_batch_score( void* runner, uint32_t count, const float* const* pcm, const uint32_t* nSamples, const int64_t* firstSample, const int64_t* countSamples,
	const int32_t* const* prompts, const uint32_t* promptCounts, const int32_t* const* tokens, const uint32_t* counts, uint32_t flags, void* const* scoresOut,
	int32_t* perRequest );
/* iContext::timingsPrint */
int32_t whisperc_timings_print( void* ctx );
/* One line of the profiler output, formatted like ProfileCollection::Measure::print (Whisper/Utils/ProfileCollection.cpp:113-170):
 * `ticks` of 100 ns scaled to seconds / milliseconds / microseconds. Returns the length written (without the terminator). */
int32_t whisperc_format_measure( const char* name, double ticks, uint64_t count, char* out, uint32_t outCap );
/* The TokenTimestamps post-processing on its own (host only, no device): token data of finished segments in, token times
 * (10 ms units) and -- with maxLen > 0 -- the segments wrapped to maxLen characters out; iContext::runFull applies exactly
 * this per segment (whisper.cpp:3374-3575, 2711-2760). segTimes / outSegTimes / outTokTimes hold (t0, t1) pairs, tokens are
 * concatenated over the segments, outTexts receives the segment texts NUL-separated. */
int32_t whisperc_debug_token_timestamps( const char* modelPath, const float* pcm, uint64_t nSamples, int32_t nSegments,
	const int64_t* segTimes, const int32_t* segTokenCounts, const int32_t* ids, const int32_t* tids, const float* p, const float* pt,
	const float* ptsum, float tholdPt, float tholdPtsum, int32_t maxLen, int32_t segCap, int32_t tokCap, int32_t* outSegCount,
	int64_t* outSegTimes, int32_t* outSegTokenCounts, char* outTexts, uint32_t textCap, int64_t* outTokTimes, float* outVlen );
/* Vocabulary and tokenizer of a model file on their own (host only, no device). whisperc_debug_tokenize returns the token count
 * (or a negative HRESULT); whisperc_debug_token_string writes the token's text and, optionally, the special ids in the order
 * eot, sot, prev, solm, not, beg, translate, transcribe (S_FALSE when the id has no string). */
int32_t whisperc_debug_tokenize( const char* modelPath, const char* text, int32_t* out, int cap );
int32_t whisperc_debug_token_string( const char* modelPath, int32_t token, char* out, uint32_t outCap, int32_t* specials8 );
/* Process-wide choice between the two host loops the reference ships: 0 (default) = its CPU model's whisper_full
 * (Whisper/source/whisper.cpp:2765-3120: drops the past prompt when < 5 s remain, retries a failed window once without it),
 * 1 = its GPU model's ContextImpl::runFullImpl (Whisper/Whisper/ContextImpl.cpp:452-793: neither rule). */
int32_t whisperc_set_host_loop_rules( int mode );
/* Where eSamplingStrategy::BeamSearch ranks a step's candidates: 0 (default) = on the device, the whole step a captured graph and the host polling
 * `done` every 16 steps (wh_beam_window_*); 1 = on the host after every step (wh_beam_candidates / wh_reorder_self_cache: the round-4 decoder, kept as
 * the checker of the device's restatement -- the two must give the same transcript). Process-wide. */
int32_t whisperc_set_beam_ranking( int onHost );
#ifdef __cplusplus
}
#endif
#endif
