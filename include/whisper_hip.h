/* whisper_hip.h -- C ABI of libwhisper_hip.so, the MI355X (gfx950) compute path.
 *
 * This is the drop-in boundary below the reference's host code: everything the reference implements in
 * Whisper/Whisper/WhisperContext.{h,cpp} (encode/decode graphs), Whisper/ML/MlContext.{h,cpp} (one method per
 * tensor op, each a D3D11 compute-shader dispatch) and the .hlsl files of ComputeShaders/ is replaced by the entry points
 * below.  Plain pointers and sizes only; no C++ types, no torch types.  All device pointers are HIP device
 * pointers; `stream` is a hipStream_t passed as void* (0 = the null stream).  Every function returns 0 on
 * success or a negative wh_status; wh_last_error() gives the text.  Nothing here ever falls back to the CPU.
 *
 * Each declaration cites the reference interface it replaces (paths relative to the reference tree).
 */
#ifndef WHISPER_HIP_H
#define WHISPER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WH_API __attribute__( ( visibility( "default" ) ) )

typedef enum wh_status
{
	WH_OK = 0,
	WH_E_INVALIDARG = -1,	/* E_INVALIDARG in the reference's HRESULT vocabulary */
	WH_E_OUTOFMEMORY = -2,
	WH_E_HIP = -3,			/* a HIP runtime call failed; see wh_last_error() */
	WH_E_NOT_READY = -4,	/* model not finalized / encode not run before decode */
	WH_E_NO_DEVICE = -5,
	WH_E_BOUNDS = -6,
	WH_E_TIMEOUT = -7		/* a collective's deadline passed: a rank did not arrive (wh_comm_create_timeout, wh_comm_set_timeout) */
} wh_status;

WH_API const char* wh_last_error( void );

/* ---- device (replaces Whisper/D3D/createDevice.cpp, listGPUs.cpp; Whisper/ML/Device.cpp:92-124) ---- */
WH_API int wh_device_count( void );
/* name: >= 256 bytes. Mirrors the adapter enumeration behind Whisper::listGPUs (Whisper/API/iContext.cl.h:62-70). */
WH_API int wh_device_info( int device, char* name, size_t nameCap, uint64_t* totalMemBytes, int* computeUnits );
WH_API int wh_device_set( int device );

/* ---- model (replaces Whisper/Whisper/ModelBuffers.{h,cpp}, WhisperModel.cpp:257-340 "loadGpu") ----
 * sModelParams of the reference (Whisper/Whisper/sModelParams.h:5-18), same field order as the ggml file. */
typedef struct wh_hparams
{
	int32_t n_vocab, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
	int32_t n_text_ctx, n_text_state, n_text_head, n_text_layer, n_mels, f16;
} wh_hparams;

typedef struct wh_model wh_model;

/* Size in bytes of the packed device weight arena for these hparams (FP16 matrices, FP32 vectors, our layout). */
WH_API int64_t wh_model_arena_bytes( const wh_hparams* hp );
/* arenaDev == NULL: the library hipMallocs the arena.  Otherwise the caller owns device memory of at least
 * wh_model_arena_bytes() bytes (e.g. a torch tensor that was just filled by an RCCL broadcast); pass
 * alreadyFilled != 0 if it already holds a finalized arena image from another rank with the same hparams. */
WH_API int wh_model_create( const wh_hparams* hp, void* arenaDev, int alreadyFilled, wh_model** out );
WH_API void wh_model_destroy( wh_model* m );
/* Upload one tensor of the ggml file by its file name ("encoder.blocks.3.attn.query.weight" ...;
 * name map Whisper/Whisper/WhisperModel.cpp:63-162).  ne[] in ggml order (ne[0] contiguous), nDims 1..3,
 * type = the ggml type of the record: 0 f32, 1 f16 (what this argument meant while it was `isF16`), or a block-quantized type of wh_dequantize below --
 * 2 q4_0, 3 q4_1, 6 q5_0, 7 q5_1, 8 q8_0 --, whose `data` is count / 32 packed blocks. A quantized matrix is loaded as the FP16 matrix of its dequantized
 * values: the blocks go to a staging buffer of the model (grown on demand, freed by wh_model_finalize and wh_model_destroy) and are expanded on the device
 * straight into the arena, which therefore holds the same bytes as after loading an f16 file with those values. Only the plain FP16 matrices -- the linear
 * layers' weights and the token embedding, ne[0] a multiple of 32 -- may be quantized; on a convolution weight, a positional embedding or a vector, and for
 * every other type number, the call fails with WH_E_INVALIDARG and names the tensor and the type.
 * `data` is HOST memory, copied synchronously.  Unknown names, wrong shapes and
 * duplicates are errors, like the reference loader (WhisperModel.cpp:292-297, 331-335). */
WH_API int wh_model_set_tensor( wh_model* m, const char* name, int nDims, const int32_t* ne, int type, const void* data );
/* ggml's block-quantized types (quantization version 2) -> FP16, on `stream`: nBlocks packed blocks of 32 elements at srcDev -> 32 nBlocks FP16 values at
 * dstDev, in order. Extends the reference, which predates quantization. Little endian, no padding between blocks; d, m FP16, qh a u32, q of element j < 16
 * the low nibble of qs[ j ] and of element j + 16 the high nibble, each with bit j resp. j + 16 of qh as its fifth bit where the type has one:
 *   type 2 q4_0  18 bytes  d, qs[16]             w = d ( q - 8 )          type 6 q5_0  22 bytes  d, qh, qs[16]       w = d ( q - 16 )
 *   type 3 q4_1  20 bytes  d, m, qs[16]          w = d q + m              type 7 q5_1  24 bytes  d, m, qh, qs[16]    w = d q + m
 *   type 8 q8_0  34 bytes  d, int8 qs[32]        w = d qs[ i ]
 * evaluated as fp16( (float)d * (float)( q - off ) ) resp. fp16( (float)d * (float)q + (float)m ): the product is exact in FP32, the sum is rounded once to
 * FP32, then to FP16 (round to nearest even). Overflow gives +-inf, a NaN d or m NaN, inf * 0 NaN; FP16 subnormals are read and written as such.
 * srcDev and dstDev must be 16-byte aligned (a workgroup's 256 blocks are then a whole number of 16-byte loads for every type; nothing outside
 * [srcDev, srcDev + nBlocks * blockBytes) is read, nothing outside the 64 nBlocks bytes at dstDev written). nBlocks == 0 is success and touches nothing.
 * WH_E_INVALIDARG, and no launch: any other type, nBlocks < 0 or >= 2^31, a null or misaligned pointer with nBlocks > 0. */
WH_API int wh_dequantize( void* stream, int type, const void* srcDev, int64_t nBlocks, void* dstDev );
/* Mel filterbank from the file header, [n_mel][n_fft] FP32 (WhisperModel.cpp:456-470). */
WH_API int wh_model_set_filters( wh_model* m, int nMel, int nFft, const float* data );
/* Verifies every expected tensor arrived exactly once (WhisperModel.cpp:331-335) and builds derived data. */
WH_API int wh_model_finalize( wh_model* m );
WH_API int wh_model_arena( wh_model* m, void** dev, int64_t* bytes );
WH_API int wh_model_hparams( const wh_model* m, wh_hparams* out );

/* ---- one process per GPU: the weights travel over xGMI (RCCL), not through every rank's file system ----
 * The reference has one GPU per model and shares a loaded model between contexts of ONE device (iModel::clone,
 * Whisper/Whisper/ModelImpl.cpp:40-60; the adapter is chosen once, API/sModelSetup.h:30-34). Windows of a recording
 * (and recordings) are independent, so N GPUs hold N copies of the arena and split the windows; the only exchange is
 * this broadcast before the first window. The communicator is RCCL's (librccl.so is opened on first use, the library
 * does not link it): rank `root` calls wh_comm_unique_id and ships the 128 bytes to the other ranks by whatever the
 * host program has (a file, a socket, MPI, an environment variable); every rank -- one process per GPU, its device
 * selected with wh_device_set -- then calls wh_comm_create with the same id. wh_model_broadcast sends the FINALIZED
 * arena of `root` into the arena of every other rank (models created with the same hparams and arenaDev == NULL or the
 * caller's own buffer) and marks those models finalized; it returns the measured seconds in *secondsOut when non-NULL. */
#define WH_COMM_ID_BYTES 128
typedef struct wh_comm wh_comm;
/* Packaging check without a GPU: the collective library opens under one of the names the entry points below try (librccl.so.1, librccl.so, the same two
 * under /opt/rocm/lib) and exports every function they call; detail (optional) receives what was opened or what is missing. 0 or WH_E_NOT_READY. */
WH_API int wh_comm_runtime_check( char* detail, size_t detailCap );
WH_API int wh_comm_unique_id( void* id128 );
WH_API int wh_comm_create( const void* id128, int rank, int worldSize, wh_comm** out );
WH_API int wh_comm_destroy( wh_comm* comm );
WH_API int wh_comm_info( const wh_comm* comm, int* rank, int* worldSize );
WH_API int wh_model_broadcast( wh_model* m, wh_comm* comm, int root, double* secondsOut );
/* All ranks: blocks until every rank has arrived (a 4-byte all-reduce on the communicator's stream). */
WH_API int wh_comm_barrier( wh_comm* comm );
/* RCCL has no deadlines: a rank that died leaves its siblings inside ncclCommInitRank / a collective for ever. With a timeout the
 * rendezvous (wh_comm_create_timeout) and every later collective of the communicator (wh_comm_set_timeout; barrier, broadcasts) return
 * WH_E_TIMEOUT after `seconds` instead; the caller is expected to give the job up (whisper-mgpu exits, its parent ends the other ranks).
 * 0 = wait for ever (wh_comm_create). */
WH_API int wh_comm_create_timeout( const void* id128, int rank, int worldSize, double timeoutSeconds, wh_comm** out );
WH_API int wh_comm_set_timeout( wh_comm* comm, double seconds );
/* Four bytes from `root` to every rank: how a root that failed BEFORE a collective (a model file it could not read) tells the ranks
 * that are about to enter it -- failure has to be collective too. */
WH_API int wh_comm_broadcast_i32( wh_comm* comm, int root, int32_t* value );

/* ---- context (replaces DirectCompute::WhisperContext, Whisper/Whisper/WhisperContext.h:20-140) ----
 * One context owns activations, the FP16 self- and cross-attention KV caches (KeyValueBuffers.h:7-53) for up to
 * maxBatch independent 30 s windows that are processed in lock step, and its workspace.  Single-threaded use,
 * like the reference (Whisper/ML/Device.cpp:163-177); several contexts of one model may be driven concurrently (each
 * has its own stream): a decode step is a chain of small dependent launches, so the work of other contexts runs
 * underneath it.  Sizing: a decode step costs about the same for 1 and for 32 windows (the weight-streaming kernel
 * holds up to 32 rows), beyond 32 the decoder falls back to the tiled GEMM; 28 windows (four 198 s clips) per context
 * and three contexts in flight is what bench.py measures. */
typedef struct wh_context wh_context;

typedef enum wh_flags
{
	WH_FLAG_NONE = 0,
	/* Emulate the reference CPU path's FP16, thread-partitioned accumulation of the decoder P.V product
	 * (Whisper/source/ggml.c:4689-4735, 4615-4644) with `parityThreads` virtual threads, and feed the encoder's P.V product
	 * the reference's operand fp16( e / sum ) (ggml.c:6035-6046) instead of the exact FP16 e with the division applied to the
	 * FP32 result. Slow; for parity runs. */
	WH_FLAG_PARITY_PV = 1,
	/* Launch the greedy loop's kernels one by one instead of replaying the captured hipGraph (debugging aid). */
	WH_FLAG_NO_GRAPH = 2,
	/* Keep copies of the intermediates at the reference's Tracing probe points (Whisper/Whisper/WhisperContext.cpp:142-638,
	 * source/whisper.cpp:1121-1869) for wh_debug_read: "enc.temp1", "enc.layer0.in", "enc-KQV", "dec-KQV", "dec-KQV#2". */
	WH_FLAG_DEBUG_CAPTURE = 4,
	/* wh_encode and wh_decode compute the reference CPU path's arithmetic IN THE REFERENCE'S SUMMATION ORDER: ggml_vec_dot_f16's 32 chains and
	 * reduction tree for every product (Whisper/source/ggml.c:751-790), sequential double sums in LayerNorm (:4098-4156), the 65536-entry GELU /
	 * exp tables, flash_attn_f16's FP16 P (:5912-6097), and the decoder's FP16 key-by-key P.V over `parityThreads` thread ranges (:4689-4735).
	 * Cross-attention caches, logits and probabilities are then the reference's BITS at that thread count (tests/test_gpu_exact.py), which is what
	 * north_star's "within 1e-3 on logits" is checked against without the reference's own thread-count band (0.05 .. 0.5 on logits) in the way.
	 * One thread per output on the VALU, no MFMA: ~100 x slower than the timed kernels, never measured. Host-stepped decoding only (wh_decode +
	 * wh_sample_best; the device-side greedy loop and beam search refuse the flag). The caches it fills are the product's own, so a timed decode
	 * step can be run on top of exact caches and vice versa. */
	WH_FLAG_PARITY_EXACT = 8
} wh_flags;

WH_API int wh_context_create( wh_model* m, int maxBatch, void* stream, wh_context** out );
/* The same with `hypotheses` decoder sequences per window (1, 2, 3, 4, 5 or 8): the sequences b*hypotheses .. b*hypotheses +
 * hypotheses-1 decode window b and share ONE pass over its cross-attention K/V per step (each has its own self-attention
 * cache). The reference declares beam search without implementing it (Whisper/API/sFullParams.h:12-13, `beam_width`,
 * `n_best`): this is the data path a beam / best-of-n decoder needs, an extension with no reference oracle beyond
 * "every hypothesis computes what a lone sequence fed the same tokens computes". In every decode entry point `batch`
 * then counts SEQUENCES (a multiple of `hypotheses`); wh_encode's `batch` keeps counting windows. */
WH_API int wh_context_create_hyp( wh_model* m, int maxBatch, int hypotheses, void* stream, wh_context** out );
WH_API void wh_context_destroy( wh_context* c );
/* Binds the model's device to the calling thread (every wh_* call on a model or context does it as well): the
 * counterpart of Device::setForCurrentThread (Whisper/ML/Device.cpp:163-177). Call it before wh_buffer_alloc /
 * wh_buffer_free, which take no context. */
WH_API int wh_context_bind( wh_context* c );
WH_API int wh_context_set_flags( wh_context* c, uint32_t flags, int parityThreads );
/* sFullParams::audio_ctx (Whisper/API/sFullParams.h; ContextImpl.cpp:24, 55, 488-489 = whisper.cpp's exp_n_audio_ctx): the encoder runs on the first
 * `audioCtx` positions of a window -- 2 * audioCtx spectrogram frames from its offset, the first audioCtx rows of the positional embedding -- and the
 * decoder's cross-attention sees that many keys. 0 = the model's n_audio_ctx. Voids the context's encoder output and captured graphs; call it between
 * windows, not between wh_encode and the decode steps that belong to it. */
WH_API int wh_context_set_audio_ctx( wh_context* c, int audioCtx );
/* Blocks until everything queued on the context's stream has finished. When `stream` was NULL at creation the context
 * owns a non-blocking stream (the legacy null stream cannot be captured into a hipGraph), so callers that produce
 * inputs or consume device outputs on another stream must order the two themselves; this is the simple way. */
WH_API int wh_context_synchronize( wh_context* c );
/* {RAM, VRAM} accounting like getMemoryUse() in the reference (WhisperContext.cpp:641-666) */
WH_API int wh_context_memory( const wh_context* c, int64_t* vramBytes );

/* Plain device buffers for host code that does not include HIP headers (PCM in, spectrogram scratch). Replaces the
 * buffer helpers of Whisper/D3D/createBuffer.cpp. upload / download are synchronous on the context's stream. */
WH_API int wh_buffer_alloc( int64_t bytes, void** dev );
WH_API int wh_buffer_free( void* dev );
WH_API int wh_buffer_upload( wh_context* c, void* dev, const void* host, int64_t bytes );
WH_API int wh_buffer_download( wh_context* c, void* host, const void* dev, int64_t bytes );
/* Enqueues the copy on the context's stream and returns; `host` must stay valid (and should be pinned) until the stream
 * passes it. This is how a caller puts the PCM upload inside the pipeline instead of in front of it. */
WH_API int wh_buffer_upload_async( wh_context* c, void* dev, const void* host, int64_t bytes );

/* PCM -> log-mel on the GPU. Replaces Spectrogram::pcmToMel (Whisper/Whisper/Spectrogram.cpp:64-122) ==
 * log_mel_spectrogram (Whisper/source/whisper.cpp:2060-2180): hop 160, Hann 400, |DFT|^2 with the reference's
 * p[j]+=p[400-j] fold, 80x201 filterbank, log10 clamp, (global max - 8) clamp, (x+4)/4.
 * pcmDev: FP32 [nSamples] device; melDev: FP32 [n_mel][nLen] device with nLen = nSamples/160 (row = mel bin).
 * The normalisation maximum is over the whole buffer, as in runFull. */
WH_API int wh_mel_spectrogram( wh_context* c, const float* pcmDev, int64_t nSamples, float* melDev, int64_t* nLenOut );

/* The same for `batch` independent buffers of nSamples each (buffer b at pcmDev + b * pcmStride -> melDev + b * melStride, each normalised by its OWN
 * maximum: what `batch` calls of wh_mel_spectrogram give, bit for bit) in three launches instead of 3 x batch -- the independent 30 s chunks of the
 * batch path (a chunk alone is 188 workgroups: less than the chip). Strides in elements; melStride >= n_mel * (nSamples / 160). */
WH_API int wh_mel_spectrogram_batch( wh_context* c, const float* pcmDev, int64_t nSamples, int64_t pcmStride, int batch, float* melDev, int64_t melStride );

/* One window of a STREAMED spectrogram. Replaces MelStreamer::makeBuffer + makeTransposedBuffer
 * (Whisper/Whisper/MelStreamer.cpp:189-245, :125-187), what iContext::runStreamed feeds the encoder with: frames
 * [frame0, frame0 + nFrames) of the stream (frame f = 400 samples from f*160, zero past nSamples; frames >= nChunks, the
 * number of 160-sample chunks the reader delivered, are 0 BEFORE normalisation), clamped to (the WINDOW's maximum - 8) with
 * the maximum floored at 1e-20, then (x+4)/4 in FP32. reusePreviousMax != 0 normalises with the maximum the previous
 * call stored instead (the streamer does that when a shorter request ends at the same frame as the last one, :158-166).
 * melDev: FP32 [n_mel][nFrames]. */
WH_API int wh_mel_spectrogram_window( wh_context* c, const float* pcmDev, int64_t nSamples, int64_t frame0, int64_t nFrames, int64_t nChunks,
	int reusePreviousMax, float* melDev );

/* PCM of any rate -> 16 kHz mono FP32 on the GPU. Replaces what the reference leaves to the OS: its Media Foundation source reader is asked for 16 kHz
 * float and resamples on the way (Whisper/MF/loadAudioFile.cpp, PcmReader.cpp). Rational polyphase resampling with a Kaiser-windowed sinc:
 *   g = gcd( inRate, 16000 ), L = 16000 / g, M = inRate / g; w = 0.9475937167399596 * min( inRate, 16000 ) / inRate; half = ceil( 32 / w ), K = 2 half + 2;
 *   h[p][k] = w sinc( w d ) I0( 14.769656459379492 sqrt( 1 - x^2 ) ) / I0( 14.769656459379492 ), d = k - half - p / L, x = d / ( half + 1 ), 0 where |x| >= 1,
 *   evaluated in double and rounded once to float;  y[n] = sum_k h[p][k] x[base - half + k], base = ( n M ) div L, p = ( n M ) mod L, x zero outside the buffer.
 * The sum runs in FP64 (one fma per tap, ascending k, one rounding to float): the correctly rounded value of the sum over the float taps up to ~1e-14.
 * Samples become floats as u8 (v - 128) / 128, s16 v / 32768, s24 v / 8388608, s32 (float)( v * 2^-31 ), f32 as is; the mean of C channels is their FP32
 * sum in channel order times 1.0f / C, taken before the filter. inRate == 16000 filters nothing: conversion and downmix only.
 * inRate 1000 .. 384000, 1 .. 8 interleaved channels, nOut == wh_resample_out_len( inRate, nFrames ) = ceil( nFrames L / M ), or WH_E_INVALIDARG;
 * nFrames == 0 is nOut == 0 and success. */
typedef enum { WH_PCM_U8, WH_PCM_S16, WH_PCM_S24, WH_PCM_S32, WH_PCM_F32 } wh_pcm_format;
/* Host only: works without a device. */
WH_API int wh_resample_out_len( int inRate, int64_t nFrames, int64_t* nOut );
/* device -> device, on `stream`; channel = -1: the mean of the channels, else that channel; dst[ n * dstStride ], dstStride 1 or 2 (interleaved stereo is
 * two calls). srcDev aligned to its sample type (s24: any). The rate's tap table is built and uploaded by the first call with that rate on the device (the
 * call waits for it) and kept for the life of the process: L * K floats -- 0.8 KB at 48 kHz, 119 KB at 44.1 kHz, 175 KB at 11.025 kHz, up to 104 MB for a rate
 * coprime to 16000 (L = 16000).
 * A workgroup owns min( 1024, ( ( 8191 - K ) L div M + 1 ) rounded down to a multiple of 64 ) consecutive outputs. */
WH_API int wh_resample( void* stream, const void* srcDev, int format, int channels, int channel, int inRate, int64_t nFrames, float* dstDev, int64_t dstStride,
	int64_t nOut );
/* host -> host on the current device: upload of the file's own samples, kernel, download. */
WH_API int wh_resample_host( const void* src, int format, int channels, int channel, int inRate, int64_t nFrames, float* dst, int64_t dstStride, int64_t nOut );
/* The same for `count` results of ONE upload (a file's mono mix and its two stereo channels): result i is channel channelList[ i ] (-1 = the mean) written to
 * dsts[ i ][ n * dstStrides[ i ] ]; the destinations may interleave in one buffer. */
WH_API int wh_resample_host_multi( const void* src, int format, int channels, const int32_t* channelList, int count, int inRate, int64_t nFrames, float* const* dsts,
	const int64_t* dstStrides, int64_t nOut );
/* the table the kernel reads: L, M, half, K and the [L][K] taps (tapsHost may be NULL to query sizes; cap = floats it holds). Host only. */
WH_API int wh_resample_taps( int inRate, int32_t* L, int32_t* M, int32_t* half, int32_t* K, float* tapsHost, int64_t cap );

/* Voice-activity features of 16 kHz mono FP32 PCM on the GPU: the per-frame half of VAD::detect (Whisper/Whisper/voiceActivityDetection.cpp:65-113; Moattar &
 * Homayounpour 2009), which the chunk planner of whisperApi.h (splitAtPauses) uses to cut a long recording at pauses. Frame f is samples [256 f, 256 f + 256),
 * the last partial frame is ignored; with x[n] = pcm[n] * 32768.0f and X the 256-point DFT of x, featDev[ 3 f .. 3 f + 2 ] =
 *   energy = sqrtf( (float)( sum_n (double)(float)( x[n] x[n] ) / 256 ) )                       the square is rounded to float, the sum is in double
 *   F      = 62.5f * the first k in 0 .. 127 that maximises |X[k]|^2                            ties go to the lower bin, an all-zero frame gives 0
 *   SFM    = -10 log10( (float)( exp( sum_{k<256} ln|X[k]| / 256 ) / ( sum_{k<256} |X[k]| / 256 ) ) )
 * The reference evaluates X with a recursive single-precision FFT over approximate sines, so its own bits are no target: the features are those of the exact
 * DFT, evaluated in FP64 (a GEMM against a host-built twiddle table on the FP64 matrix cores, fixed summation order) and rounded once to float; sqrtf and the
 * final log10 are the correctly rounded float functions. A frame's numbers depend on its 256 samples only: not on the buffer's length, its address or the
 * frame's place in a workgroup (16 frames each).
 * Special values: an all-zero frame has energy 0, F 0 and SFM NaN (0 / 0). A frame with a bin that vanishes exactly has SFM +inf in exact arithmetic; the
 * device returns +inf where its own sum for that bin is exactly zero (bins 0 and 128, whose twiddles are +-1: the alternating or the plain sum of
 * integer-valued samples is exact) and otherwise a FINITE number: the bin's rounding noise, about 1e-16 of the frame's norm, stands in for the zero, and
 * ln of it is about -37 instead of -inf, which lifts SFM by some 10 log10( e ) 2 * 37 / 256 = 1.3 dB over what the other bins give. A bin that cancels
 * exactly against irrational twiddles takes samples constructed for it (a frame of two equal halves, say); recorded audio does not do that.
 * nSamples < 256 gives zero frames and success; null or misaligned pointers with nFrames > 0, nSamples < 0 or > 2^40: WH_E_INVALIDARG.
 * The twiddle table (4 KB) is built and uploaded by the first call on a device (the call waits for it) and kept for the life of the process. */
/* Host only: *nFrames = nSamples / 256. */
WH_API int wh_vad_frame_count( int64_t nSamples, int64_t* nFrames );
/* device -> device, on `stream`; featDev: FP32 [nFrames][3] */
WH_API int wh_vad_features( void* stream, const float* pcmDev, int64_t nSamples, float* featDev );
/* host -> host on the current device: upload of the whole frames, kernel, download. */
WH_API int wh_vad_features_host( const float* pcm, int64_t nSamples, float* feat );

/* Speech only: the spans of a recording that hold speech, packed one behind the other (Whisper::setSpeechFilter of whisperApi.h).
 * wh_speech_pack: device -> device, on `stream`: dst[ out[i] + k ] = src[ a_i + k ] for k < b_i - a_i, where spans (HOST, int64 [count][2]) holds a_i, b_i in
 * sample frames and out[i] is the total length of the spans before i; a frame is `channels` (1 or 2, interleaved) FP32 values. A bit copy: NaN payloads
 * survive, nothing is converted. The spans must be non-empty, ascending, disjoint and inside [0, nSamples], count <= 65536, nOut their total length, the
 * buffers non-null and 4-byte aligned: anything else is WH_E_INVALIDARG with no launch; count == 0 succeeds with no launch. The table of count + 1 output
 * offsets and count span starts goes to device memory behind what the stream holds, the launch behind it, and the call returns when both are done (the
 * table is the call's own). A workgroup owns 16384 consecutive output values, finds its first span with one binary search and walks on; where both sides of
 * a span are 16-byte aligned -- always, for spans of the span rules (multiples of 256 samples) in buffers of hipMalloc -- the body moves 128-bit vectors and
 * only the tail of the last span single values; other spans are copied value by value. Nothing outside [0, nOut * channels) of dstDev is written. */
WH_API int wh_speech_pack( void* stream, const float* srcDev, int channels, int64_t nSamples, const int64_t* spans, int count, float* dstDev, int64_t nOut );
/* host -> host on the current device: upload, kernel, download. */
WH_API int wh_speech_pack_host( const float* src, int channels, int64_t nSamples, const int64_t* spans, int count, float* dst, int64_t nOut );
/* The whole filter on a context's stream: wh_vad_features on pcmDev (16 kHz mono FP32, nSamples), the download of the features (12 bytes per 256-sample
 * frame), the reference's decision loop and the span rules on the host (host/vad.h, host/speechSpans.h; params in frames, 0 or params == NULL = the defaults
 * 125 / 16 / 25), then the pack kernel for the mono buffer and, if stereoDev (interleaved, nSamples frames) is given, for the stereo buffer. The call waits
 * for the stream. spansOut [cap][2] receives the *count spans (WH_E_BOUNDS when cap is too small; *count is set), *nPacked their total length.
 * *packedDev / *packedStereoDev (the latter may be NULL) are buffers of the context, valid until the next call or the context's end; the first call that
 * needs them allocates them. No span: *packedDev = NULL, *nPacked = 0. One span that covers [0, nSamples): *packedDev = pcmDev (and the stereo likewise) and
 * nothing is launched behind the features. A context that never calls this allocates and launches nothing of it. */
typedef struct { int32_t minSilenceFrames, minSpeechFrames, padFrames; } wh_speech_params;
WH_API int wh_context_speech_filter( wh_context* c, const float* pcmDev, int64_t nSamples, const float* stereoDev, const wh_speech_params* params,
	const float** packedDev, const float** packedStereoDev, int64_t* nPacked, int64_t* spansOut, int cap, int* count );

/* A live PCM stream, chunk by chunk: the buffer of the capture loop of iContext::runCapture (Whisper/Whisper/ContextImpl.capture.cpp: readSample appends
 * the converted samples, detectVoice looks at the whole buffer). A wh_capture is made for 1 or 2 input channels at 16 kHz (another rate: below) and owns, each for capSamples
 * samples: a device buffer of mono FP32, with keepStereo one of interleaved stereo FP32, and a pinned host mirror of both -- twice, see wh_capture_take.
 * It has a stream of its own (the context only names the device), so an append never waits for a transcription that runs on a context's stream.
 * A context that never captures allocates and launches nothing of this.
 *
 * wh_capture_append: src (HOST) holds `frames` interleaved sample frames of the capture's channel count in `format`, WH_PCM_S16 or WH_PCM_F32. One upload of
 * the chunk in its own format, ONE kernel launch, one download of the features; the call waits for the capture's stream only. With n the samples buffered:
 *   - samples [n, n + frames) of the mono buffer, of the stereo buffer if kept and of the mirror are written by wh_resample's rules for inRate == 16000:
 *     s16 is v / 32768, f32 as is; mono of two channels is the FP32 sum in channel order times 0.5f; a mono source whose stereo is kept gets its channel twice;
 *   - featHost [nNewFrames][3] receives the voice-activity features of the 256-sample frames the chunk completes, frames [n / 256, ( n + frames ) / 256) of the
 *     buffer -- a frame that began in an earlier chunk takes its older samples from the buffer --, with the bits wh_vad_features gives for the same 256 samples:
 *     both kernels call the same device function (csrc/vad_device.h).
 * A workgroup owns 16 consecutive frames of buffer positions, as in wh_vad_features: it converts the part of the chunk that falls into them, then computes the
 * features of the frames among them that the chunk completes. WH_E_BOUNDS, and no launch, when the chunk does not fit; WH_E_INVALIDARG, and no launch, for
 * another format, a null pointer with frames > 0, or featCap (frames of 3 floats) below the number of completed frames. frames == 0 succeeds with no launch.
 * wh_capture_clear empties the buffer: position 0, no partial frame. wh_capture_take hands out the host mirror of what is buffered (stereoHost receives NULL
 * when stereo is not kept; the argument itself may be NULL) and empties the buffer; the mirror is two buffers that swap, so what was handed out stays valid
 * until the take after the next (the reference's pcm.swap( buffer.pcm )): the piece under transcription is not overwritten while the next one fills.
 * One thread at a time per capture.
 *
 * A stream at another rate: wh_capture_create_rate, inRate 1000 .. 384000 Hz (16000 gives exactly the object wh_capture_create gives). The chunk is resampled
 * by the same launch with wh_resample's filter made resumable, and the contract is: the 16 kHz samples such a capture ever puts into its buffer are, in order,
 * the samples wh_resample gives for the whole stream at once, bit for bit, whatever the chunk sizes. With L, M, half, K of wh_resample_taps( inRate ), the
 * stream holds nIn (input frames accepted), nOut (outputs emitted or skipped), z (frames below it read as zero) and the last K - 1 frames of every filtered
 * channel (the FP32 downmix; channels 0 and 1 as well when the stereo of a two-channel source is kept; a mono source whose stereo is kept gets its one
 * filtered channel twice):
 *   - wh_capture_append: `frames` are INPUT frames. nIn += frames; the outputs [nOut, max( nOut, ready )), ready = max( 0, ceil( ( nIn - half - 1 ) L / M ) ),
 *     are appended at n -- those whose last tap lies inside what has arrived, so the look-ahead is half + 1 input frames (2.1 to 2.2 ms from 22.05 kHz up,
 *     3.2 ms at 11.025 kHz, 4.4 ms at 8 kHz). A small chunk may append nothing; the caller learns what was appended from wh_capture_size. featHost must hold
 *     the frames that ceil( frames L / M ) + 1 outputs can complete.
 *   - wh_capture_flush, at the end of the stream: the outputs [nOut, ceil( nIn L / M )) are appended with zeros behind the last frame; the total is then
 *     wh_resample_out_len( inRate, nIn ). The same launch with half + 1 frames of zeros for a chunk; no launch when nothing is left. Afterwards append, flush
 *     and skip answer WH_E_NOT_READY.
 *   - wh_capture_skip: `frames` input frames that the caller discarded (a stalled capture loop) are counted without an upload or a launch: nIn += frames,
 *     nOut = max( nOut, ceil( nIn L / M ) ), z = nIn; *nSkippedOutputs is by how much nOut grew. What is appended afterwards are the samples of wh_resample
 *     over the stream with frames [0, z) set to zero, from output ceil( z L / M ) on.
 *   - wh_capture_clear and wh_capture_take reset the buffer position only: nIn, nOut, z and the history belong to the stream and go on.
 * On a 16 kHz capture flush appends nothing and skip answers `frames`. */
typedef struct wh_capture wh_capture;
WH_API int wh_capture_create( wh_context* c, int channels, int keepStereo, int64_t capSamples, wh_capture** out );
WH_API int wh_capture_create_rate( wh_context* c, int channels, int keepStereo, int64_t capSamples, int inRate, wh_capture** out );
WH_API int wh_capture_flush( wh_capture* cap, float* featHost, int64_t featCap, int64_t* nNewFrames );
WH_API int wh_capture_skip( wh_capture* cap, int64_t frames, int64_t* nSkippedOutputs );
WH_API int wh_capture_append( wh_capture* cap, const void* src, int format, int64_t frames, float* featHost, int64_t featCap, int64_t* nNewFrames );
WH_API int wh_capture_clear( wh_capture* cap );
WH_API int wh_capture_take( wh_capture* cap, const float** monoHost, const float** stereoHost, int64_t* nSamples );
WH_API int wh_capture_size( const wh_capture* cap, int64_t* nSamples );
/* 0 or WH_E_BOUNDS when a guard region of a device buffer was written (WH_DEBUG_POISON) */
WH_API int wh_capture_destroy( wh_capture* cap );

/* Encoder. Replaces WhisperContext::encode (WhisperContext.cpp:310-399) == whisper_encode (whisper.cpp:1084-1496).
 * melDev: FP32 device, `batch` spectrograms each [n_mel][melLen] (melStride floats apart); for each the window
 * [melOffset, melOffset + 2*n_audio_ctx) is taken and zero-padded (MelInputTensor.cpp:8-63).  Fills the
 * cross-attention caches of all decoder layers for batch slots 0..batch-1 and resets their self-attention state. */
WH_API int wh_encode( wh_context* c, const float* melDev, int batch, int64_t melLen, int64_t melStride, const int32_t* melOffsets );

/* The same for windows that come from DIFFERENT spectrograms (recordings of different lengths: the streams of Whisper::runFullBatch):
 * window b = frames [offset, offset + 2*n_audio_ctx) of the FP32 [n_mel][melLen] spectrogram at melDev, zero beyond its end
 * (MelInputTensor.cpp:8-63); melDev == NULL is a window of zeros (an idle slot of a lock-step batch). windows: HOST [batch]. */
typedef struct wh_mel_window
{
	const float* melDev;
	int64_t melLen;
	int32_t offset, reserved;
} wh_mel_window;
WH_API int wh_encode_windows( wh_context* c, const wh_mel_window* windows, int batch );

/* Decoder step. Replaces WhisperContext::decode (WhisperContext.cpp:578-639) == whisper_decode (whisper.cpp:1508-1872).
 * tokens: HOST int32 [batch][nTokens]; every sequence advances from position nPast by nTokens.
 * Outputs for the LAST token of each sequence (the only row the reference ever consumes, ContextImpl.cpp:159-169):
 *   logitsHost / probsHost: HOST FP32 [batch][n_vocab], either may be NULL (skips that download).
 * Synchronises the stream before returning when any host output is requested. */
WH_API int wh_decode( wh_context* c, const int32_t* tokens, int batch, int nTokens, int nPast, float* logitsHost, float* probsHost );

/* Language detection. Replaces whisper_lang_auto_detect (Whisper/source/whisper.cpp:2428-2495; the reference's GPU model has none).
 * After wh_encode / wh_encode_windows of at least `batch` windows: one decoder step of [sot] at position 0 for windows 0 .. batch-1, then for every window
 * the probabilities of the language tokens sot + 1 .. sot + n_lang under the full-vocabulary softmax -- what wh_decode's probsHost holds at those columns,
 * bit for bit (under WH_FLAG_PARITY_EXACT: the reference's own bits) -- and the index of the largest (ties to the lower id). The [batch][n_vocab] rows are
 * never written or downloaded on the timed path. The reference's lang_probs are a SECOND softmax over these numbers (exp( p ) / sum exp( p )), which the
 * caller applies on the host if it wants them.
 * langP: HOST [batch][n_lang] (may be NULL), best: HOST [batch]. Leaves the sequences as wh_encode left them, so the windows can be decoded right away
 * without being encoded again. The probabilities wh_sample_best / wh_beam_candidates read belong to the last wh_decode and are UNDEFINED after this
 * call (the timed path never writes the step's full rows): decode before sampling again. On a hypothesis-group context `batch` counts windows. WH_E_INVALIDARG on a model that is not multilingual. */
WH_API int wh_lang_detect( wh_context* c, int batch, float* langP, int32_t* best );
/* Language tokens of the model's vocabulary: n_vocab - 51766 (99 at 51865, 100 at the large-v3 shape), 0 for .en models. */
WH_API int wh_model_lang_count( const wh_model* m );

/* Token alignment: word-level timestamps from the decoder's cross-attention by dynamic time warping, as openai-whisper's word_timestamps and
 * whisper.cpp's --dtw do it (an extension: the reference has the TokenTimestamps heuristic only). The definition is DESIGN.md "Token alignment",
 * restated in numpy by tests/align_ref.py.
 *   wh_model_set_alignment_heads: the heads whose weights are averaged, `count` (layer, head) pairs; they are used in ascending (layer, head) order and a
 *     pair named twice counts once. count == 0 restores the default: every head of decoder layers n_text_layer / 2 .. n_text_layer - 1.
 *   wh_align_tokens: after wh_encode / wh_encode_windows of at least `batch` windows and after their decoding is over (the call overwrites the sequences' self-
 *     attention caches, decoder activations, logits and probabilities). tokens: HOST [batch][nMax], row b = the lens[ b ] tokens
 *     [sot sequence, no-timestamps token, text ..., eot] followed by padding (ignored); the text begins behind the row's first no-timestamps token, at least one
 *     text token, 3 <= lens[ b ] <= nMax <= min( 256, n_text_ctx ). nKeys: HOST [batch], the keys (audio positions of 20 ms) of window b that take part,
 *     1 .. the context's audio context. One teacher-forced pass of the multi-token decoder graph at position 0, ended behind the cross-attention query of the
 *     last selected layer (the debug captures of WH_FLAG_DEBUG_CAPTURE are left as the last wh_decode made them); the matrix and the DTW run on the device and only the frames come back:
 *     framesHost: HOST [batch][nMax], row b = for each text token and then the eot row the smallest key index of the warping path inside its row
 *     (lens[ b ] - 1 - p numbers, p = the index of the no-timestamps token), then -1. Frames of a row never decrease.
 *     The matrix and DTW kernels give a window the same bits whatever the batch, its place in it and nMax; the pass before them is the decoder's own, which
 *     picks its product kernels by the total number of rows, so a window's FP16 query rows may move in their last bits with the batch. Greedy contexts only: WH_E_INVALIDARG on a
 *     hypothesis-group context and under WH_FLAG_PARITY_EXACT. Buffers are allocated by the first call; contexts that never call it pay nothing.
 * wh_debug_read: "align-matrix" = the last call's M, [batch][nMax][audio context] (zero outside a window's rows and keys); "align-q" = the FP16 cross-attention
 *     query rows of `layer` (one of the selected heads' layers) as that pass formed them, [batch * nMax][d]. */
WH_API int wh_model_set_alignment_heads( wh_model* m, const int32_t* layerHeadPairs, int count );
WH_API int wh_align_tokens( wh_context* c, int batch, const int32_t* tokens, const int32_t* lens, const int32_t* nKeys, int nMax, int32_t* framesHost );

/* Scoring a GIVEN transcript: teacher-forced token log-probabilities (an extension: the reference only scores what it samples). The definition is DESIGN.md
 * section 7 "Scoring", restated in float64 by tests/token_score_ref.py. A row of FP32 logits x[ 0 .. V ) and a target id t give one record:
 *   logprob     = x[ t ] - m - ln sum_j exp( x[ j ] - m ), m = max_j x[ j ];
 *   bestLogprob = -ln sum_j exp( x[ j ] - m ), the log-probability of the arg-max;
 *   best        = the lowest id j with x[ j ] == m;
 *   rank        = #{ j : x[ j ] > x[ t ] } + #{ j < t : x[ j ] == x[ t ] }: 0 means t is what an arg-max would take under wh_sample_best's tie rule (exact ties
 *                 resolve to the lower token id).
 * These are TRUE logarithms, not ln of the table softmax's probabilities (whose FP16 exponential is 0 for an unlikely token): FP32 expf per term, the sum in
 * double, the two logarithms formed in double and rounded once. An entry of -inf adds 0 to the sum; a target at -inf scores -inf with a finite bestLogprob.
 * The pass scores the model's OWN distribution: neither the suppressed set (wh_context_set_suppress) nor the timestamp rules nor any clause of wh_sample_best
 * applies, as in wh_lang_detect.
 *   wh_score_tokens: after wh_encode / wh_encode_windows of at least `batch` windows and after their decoding is over (the call overwrites the sequences' self-
 *     attention caches and the decoder activations like wh_align_tokens; logits and probabilities of the last wh_decode stay as they were, the product writes into a
 *     buffer of its own). tokens: HOST [batch][nMax], row b = lens[ b ] tokens followed by padding (ignored). Entry i of row b is scored for
 *     firstScored[ b ] <= i < lens[ b ], 1 <= firstScored[ b ] < lens[ b ] <= nMax <= min( 256, n_text_ctx ): the probability of token i given tokens 0 .. i - 1,
 *     that is, decoder row i - 1. One teacher-forced pass of the multi-token decoder graph at position 0 through every layer and the final LayerNorm; the needed
 *     rows are gathered compactly and go through the vocabulary product at most "score_chunk_rows" rows at a time, each chunk reduced by the kernel of
 *     wh_op_token_scores, so the [rows][n_vocab] logits are never downloaded. The product is the M-tiled kernel whatever the row count, so the records do not
 *     depend on the chunk size, bit for bit. The pass before it is the decoder's own, which picks its kernels by the total number of rows: a window's records
 *     may move in their last bits with the batch. outHost: HOST [batch][nMax], the scored entries filled, every other one zero.
 *     Greedy contexts only: WH_E_INVALIDARG on a hypothesis-group context and under WH_FLAG_PARITY_EXACT. Buffers are allocated by the first call; contexts that
 *     never call it pay nothing, and no captured graph changes. */
typedef struct wh_token_score
{
	float logprob, bestLogprob;
	int32_t best, rank;
} wh_token_score;
WH_API int wh_score_tokens( wh_context* c, int batch, const int32_t* tokens, const int32_t* lens, const int32_t* firstScored, int nMax, wh_token_score* outHost );

/* sTokenData of the reference (Whisper/Whisper/sTokenData.h): the result of ContextImpl::sampleBest. */
typedef struct wh_token_data
{
	int32_t id, tid;
	float p, pt, ptsum;
} wh_token_data;

/* Greedy sampling on the device, from the probabilities of the last wh_decode call. Replaces
 * ContextImpl::sampleBest / sampleTimestamp (Whisper/Whisper/ContextImpl.cpp:71-169): timestamp-vs-text rule,
 * initial-timestamp <= 1.00 s cap, first of the top-4 that is not sot/solm/not. forceTimestamp / isInitial are
 * per call (same for all sequences). out: HOST [batch]. Exact ties resolve to the lower token id. */
WH_API int wh_sample_best( wh_context* c, int batch, int forceTimestamp, int isInitial, wh_token_data* out );

/* Beam search on hypothesis groups (extension: the reference declares eSamplingStrategy::BeamSearch / beam_search.beam_width,
 * Whisper/API/sFullParams.h:10-13, and implements only the greedy strategy). Data path of one step, for the sequences of a
 * wh_context_create_hyp context:   wh_decode( tokens, batch, 1, nPast, NULL, NULL )  ->  wh_beam_candidates  ->  the host ranks
 * parent score + log p over each window's candidates and keeps the best `hypotheses`  ->  wh_reorder_self_cache( parents )  ->  next wh_decode.
 *   wh_beam_candidates: the `width` (1 .. 8) best continuations of every sequence from the probabilities of the last wh_decode, under
 *     sampleBest's own rules (timestamp-vs-text sum rule, initial-timestamp cap, sot / solm / not skipped): candidate 0 IS wh_sample_best's
 *     token, so width 1 is the greedy decoder. out: HOST [batch][width].
 *   wh_reorder_self_cache: sequence j continues sequence parents[j] (same window): rows [0, rows) of the self-attention caches of all layers are
 *     copied parents[j] -> j (through a scratch copy, so any permutation is safe; parents[j] == j costs nothing). The cross-attention K/V of a
 *     window are shared by its hypotheses and never move. */
WH_API int wh_beam_candidates( wh_context* c, int batch, int width, int forceTimestamp, int isInitial, wh_token_data* out );
WH_API int wh_reorder_self_cache( wh_context* c, int batch, const int32_t* parents, int rows );

/* Beam search WITHOUT the host in the loop (round 5; configs[2] of BASELINE.json). The per-step ranking above -- pool of live hypotheses x candidates
 * by parent score + log p, the best `width` accepted, the window's stop rules applied to each (WindowScan of libWhisper.so's host loop =
 * Whisper/Whisper/ContextImpl.cpp:597-673), finished / live lists, "can a live hypothesis still win" -- runs as a kernel behind every decode step,
 * writes the parents the next step's cache reorder reads and the tokens its embedding reads, and the whole step (reorder -> decode -> softmax ->
 * candidates -> ranking) is ONE captured graph replayed per token. The host enqueues chunks of steps and polls `done`.
 *   wh_beam_window_start    windows x (hypotheses of the context) sequences; promptTokens HOST [windows][nPrompt] (every slot of a window starts from
 *                           it); rules HOST [windows]; the prompt step, the first ranking (sampleTimestamp( true ) rules) and nSteps ranked steps are
 *                           enqueued. The call WAITS for what the stream holds first (the window's rules and initial state are copied synchronously, and the step
 *                           graph is captured on first use): one host round trip per window, the encoder included; the steps themselves never block. The
 *                           captured graph is keyed on (sequences, width) and on what the greedy step's is (the parity mode, "a suppressed set is held"): kernel options set with wh_debug_set_option / _tuning afterwards do not reach it.
 *                           forced != 0 in a window's rules: no stop rules, every hypothesis lives (random-weight workloads).
 *   wh_beam_window_continue nSteps more (bounded by n_text_ctx like wh_decode_window_continue). Steps enqueued after a window is done change nothing.
 *   wh_beam_window_status   blocks until everything enqueued has run; the search state of every window: HOST [windows].
 *   wh_beam_window_records  the accepted proposals of ranking steps [firstStep, firstStep + count): HOST [count][windows][width]; a hypothesis' token
 *                           chain is followed from its `rec` (= step * width + index) through `parent` down to -1 (parent == -2: unused entry).
 * Width 1 is the greedy decoder token for token. */
typedef struct wh_beam_rules
{
	int32_t seek, seekEnd;		/* the window's first frame and the stream's end, 10 ms units */
	int32_t nMax;				/* n_text_ctx / 2 - 4 */
	int32_t maxTokens;			/* sFullParams::max_tokens (0 = no limit) */
	int32_t singleSegment;
	int32_t tokenBeg, tokenEot;
	int32_t forced;
} wh_beam_rules;
typedef struct wh_beam_hyp
{
	double sum;					/* cumulative log-probability */
	int32_t i, hasTs, seekDelta, resultLen, failed, over;	/* WindowScan's state */
	int32_t nTok, rec;
} wh_beam_hyp;
typedef struct wh_beam_window
{
	int32_t step, nLive, nFinished, done;
	int32_t nPrompt, nTextCtx, reserved0, reserved1;
	wh_beam_hyp live[ 8 ];
	wh_beam_hyp finished[ 24 ];
} wh_beam_window;
typedef struct wh_beam_record
{
	wh_token_data t;
	int32_t parent, finished, reserved;
} wh_beam_record;
WH_API int wh_beam_window_start( wh_context* c, int windows, const int32_t* promptTokens, int nPrompt, int width, const wh_beam_rules* rules, int nSteps );
WH_API int wh_beam_window_continue( wh_context* c, int nSteps );
WH_API int wh_beam_window_status( wh_context* c, wh_beam_window* out );
WH_API int wh_beam_window_records( wh_context* c, int firstStep, int count, wh_beam_record* out );

/* The greedy loop of ContextImpl::runFullImpl (Whisper/Whisper/ContextImpl.cpp:597-673: decode -> sampleBest ->
 * feed the token back) kept on the device for nSteps tokens: firstTokens (HOST, [batch]) are fed at position nPast, each
 * step runs the decoder for one token per sequence, samples with the sampleBest rules and feeds the choice back, with
 * no host round trip in between (one captured hipGraph is replayed per token; position and flags live in device
 * memory). forceFirstTimestamp / firstIsInitial apply to the first sample only (sampleTimestamp(true) of the
 * reference). out: HOST [nSteps][batch]. The host applies its stop rules to the returned tokens afterwards; tokens
 * sampled after a sequence's stop condition are simply discarded by the caller. */
WH_API int wh_decode_greedy( wh_context* c, int batch, const int32_t* firstTokens, int nPast, int nSteps, int forceFirstTimestamp,
	int firstIsInitial, wh_token_data* out );

/* One whole window's decode, enqueued without blocking the host: prompt step (HOST tokens [batch][nPrompt] at position 0)
 * -> first sample -> nSteps greedy steps; wh_decode_window_finish blocks and returns the 1 + nSteps samples as HOST
 * [1 + nSteps][batch]. Contexts own their streams, so several windows (or groups of windows) started back to back from
 * one host thread overlap on the GPU: a single-token decode step is latency-bound and occupies a fraction of the CUs. */
WH_API int wh_decode_window_start( wh_context* c, int batch, const int32_t* promptTokens, int nPrompt, int nSteps, int forceFirstTimestamp,
	int firstIsInitial );
WH_API int wh_decode_window_finish( wh_context* c, wh_token_data* out );
/* The same for a lock-step batch whose sequences carry prompts of DIFFERENT lengths -- the streams of a batch scheduler (Whisper::runFullBatch
 * of libWhisper.so): every stream keeps the reference's sequential semantics, so its window's prompt is [prev] + its own past text + the task
 * tokens (ContextImpl.cpp:565-576) and the streams of one batch stand at different decoder positions. promptTokens: HOST [batch][nPromptMax],
 * row b = promptLens[b] tokens followed by padding (ignored); 1 <= promptLens[b] <= nPromptMax. Sequence b then computes exactly what it computes
 * alone: its tokens sit at positions 0 .. promptLens[b]-1, its greedy step s feeds position promptLens[b] + s, its self-attention sees its own
 * keys only (positions live per sequence in device memory; the padded rows of a shorter prompt are computed and never consumed: their cache
 * rows are overwritten by the sequence's own later tokens before any query can see them). One hypothesis per window.
 * nPromptMax + nSteps (and every later wh_decode_window_continue) is bounded by n_text_ctx. */
WH_API int wh_decode_window_start_ragged( wh_context* c, int batch, const int32_t* promptTokens, const int32_t* promptLens, int nPromptMax, int nSteps,
	int forceFirstTimestamp, int firstIsInitial );
/* nSteps more greedy steps of the window in progress (no host round trip: position, last token and sampler flags are in
 * device memory), and a blocking read of samples [first, first + count) -> HOST [count][batch] that waits for those
 * samples only. The reference's loop looks at every token before it decodes the next one (ContextImpl.cpp:597-673); a
 * caller that keeps one chunk queued behind the one it is scanning loses at most that chunk when a stop token shows up. */
WH_API int wh_decode_window_continue( wh_context* c, int nSteps );
WH_API int wh_decode_window_fetch( wh_context* c, int first, int count, wh_token_data* out );
/* Non-blocking: 1 when samples [first, first + count) of the window in progress exist (wh_decode_window_fetch would not wait), 0 when not
 * yet, negative on error. Lets ONE host thread serve several contexts (a scheduler that keeps two lock-step batches in flight). */
WH_API int wh_decode_window_ready( wh_context* c, int first, int count );

/* Temperature sampling in the device-side loop (wh_decode_greedy, wh_decode_window_*). temperature == 0 -- the state of every new context -- is the greedy
 * sampler. With temperature > 0 every sample, the prompt step's first one under its forceTimestamp / isInitial flags included, is
 * wh_op_vocab_soft_max_scaled( invT = 1.0f / temperature ) followed by wh_op_sample_draw with the sequence's decoder position (the position of the token that
 * was just fed: prompt length - 1 for the first sample) and this seed and nonce. The values are stored in device memory behind what the stream holds (the call
 * waits for the stream), and the captured step graph is keyed on the mode, not on the values: an attempt at another temperature or nonce replays the same graph,
 * going back to 0 replays a greedy graph. WH_E_INVALIDARG for a temperature that is negative, NaN or above 4, and, above 0, on a hypothesis-group context or
 * under WH_FLAG_PARITY_EXACT. A context that never calls it launches, allocates and captures what it always did. */
WH_API int wh_context_set_sampling( wh_context* c, float temperature, uint64_t seed, uint32_t nonce );
/* Per-row sampling for a lock-step batch (wh_decode_window_start_ragged and its chunks) whose sequences stand at different attempts: sequence r of every
 * following step is greedy where temperature[ r ] == 0 and otherwise samples at temperature[ r ] in (0, 4] under its own Philox key seed[ r ] and nonce[ r ];
 * sequences beyond `rows` are greedy. HOST arrays [rows], 1 <= rows <= the context's sequences. Every step is then two one-workgroup-per-row kernels, whatever
 * the batch: the table softmax of logits * ( 1 / T ) with the factor read per row (1.0f for a greedy row: x * 1.0f is x, the greedy probabilities bit for bit),
 * and a draw kernel that gives a greedy row wh_op_sample_best's record and a sampled row wh_op_sample_draw's record for that row ALONE -- the Philox counter is
 * ( position, 0, nonce[ r ], 0 ), so a stream's draws do not depend on the slot it sits in. The records are uploaded through pinned staging behind what the
 * stream holds (work queued earlier still reads the old ones; the call does not wait for the stream). The mode has a captured step graph of its own, which
 * lives next to the greedy one: entering and leaving the mode recaptures nothing. rows == 0, or every temperature 0, turns the mode off: the greedy sampler
 * and graph, exactly what a context that never made the call launches (at <= 4 sequences that is the spread sampler, whose ptsum may differ from a greedy row
 * of a per-row step in the last bits of a double sum). wh_context_set_no_speech gathers probabilities in this mode as in the others.
 * WH_E_INVALIDARG on a hypothesis-group context, under WH_FLAG_PARITY_EXACT, for a vocabulary above 65536, for a temperature that is NaN or outside [0, 4],
 * and while wh_context_set_sampling has a temperature set (which in turn refuses a temperature while this mode is on). */
WH_API int wh_context_set_sampling_rows( wh_context* c, int rows, const float* temperature, const uint64_t* seed, const uint32_t* nonce );
/* The model's own "no speech" probability of a window: when on, wh_decode_window_start / _start_ragged queue one small gather behind the prompt step's sample,
 * p[ token_solm ] of every sequence's row of probabilities as that step formed it (the id the reference calls token_solm, 50361 + 1 when multilingual, is
 * <|nospeech|> in OpenAI's vocabulary). wh_decode_window_no_speech: HOST float [batch] of the window in progress; waits for the first sample only. The buffer
 * is allocated by the first call that turns it on. */
/* Suppressed tokens, openai-whisper's definition: the logits of these ids are replaced by -inf before the softmax, for every row of every later decoder pass of
 * the context -- wh_decode (the logits and probabilities it returns included), the greedy, tempered and per-row steps of the device-side loop, the prompt step's
 * first sample, the beam step -- by ONE small launch behind the vocabulary product; no sampler changes, each reads -inf as probability 0. Two passes stay
 * unfiltered: wh_lang_detect (the model's own distribution at [sot], the same bits whatever set is held) and wh_align_tokens (which forms no logits). The
 * no-speech gather reads the row the sampler saw: with a set held it is the filtered distribution's probability.
 * ids: HOST [count], each in [0, eot) -- text tokens only, so every row keeps mass; duplicates allowed, the sorted unique set is stored. count == 0 (ids may be
 * NULL) is the state of every new context. The set goes to device memory behind what the stream holds (the call waits for the stream); the buffer, eot + 1 int32,
 * is allocated by the first non-empty call and never again, and the captured step graphs are keyed on "a set is held" only: another set replays the same graph.
 * WH_E_INVALIDARG for an id outside the range and for a non-empty set under WH_FLAG_PARITY_EXACT (wh_context_set_flags in turn refuses that flag while a set is
 * held). Hypothesis-group contexts take the call like greedy ones. A context that never calls it launches, allocates and captures what it always did. */
WH_API int wh_context_set_suppress( wh_context* c, const int32_t* ids, int count );
/* Timestamp rules: the three clauses of openai-whisper's ApplyTimestampRules that the sampler does not hold, as -inf over ranges of the logits, for every row of
 * every later step of the device-side loop. A token is a timestamp when its id is >= beg (<|0.00|>). (1) Pairs: after `text, <|t|>` the next token is a timestamp
 * or eot ([0, eot) is masked; eot and the special ids stay, so a row always keeps mass); after `<|t|>, <|t|>` it is no timestamp ([beg, nVocab) is masked; "the
 * one before" also counts as a timestamp while fewer than two tokens have been sampled). (2) No timestamp below the last one sampled in this window and (3) none
 * equal to it either, unless it closes a pair: [beg, last) is masked in the text-then-timestamp case, [beg, last + 1) otherwise. The sampler's own two clauses (the
 * timestamp mass against the best text token, the first timestamp's cap) are unchanged and see the filtered row.
 * The mask depends on what the row has sampled, so the context keeps one record of four int32 per sequence in device memory (last token a timestamp, the one
 * before it, the last timestamp id, tokens sampled). ONE small launch behind the vocabulary product folds the token just fed -- the previous step's sample -- into
 * the record and masks the row; the prompt step of a window resets the records and masks nothing, so the window's first sample is what it always was and no
 * record survives into the next window. It applies to wh_decode_greedy (the history starts at the call's first sample: firstTokens are not counted),
 * wh_decode_window_start, _start_ragged and _continue, whatever the sampler: greedy, wh_context_set_sampling, wh_context_set_sampling_rows. Unfiltered: wh_decode
 * (the host feeds the tokens, there is no device history), wh_lang_detect, wh_align_tokens and the beam step.
 * The records, maxSeq of them, are allocated by the first call that turns the mode on and never again; the captured step graphs are keyed on the mode. The call
 * waits for the stream: what was queued runs under the mode it was queued in. WH_E_INVALIDARG to turn it on on a hypothesis-group context (the records would have
 * to follow the beam's reorder) or under WH_FLAG_PARITY_EXACT (wh_context_set_flags in turn refuses that flag while the mode is on). A context that never turns
 * it on launches, allocates and captures what it always did. */
WH_API int wh_context_set_timestamp_rules( wh_context* c, int on );
/* Phrase boosting ("hotwords"; DESIGN.md section 7 "Phrase boosting" holds the definition). A context holds a set of phrases -- each 1 .. 16 text-token ids in
 * [0, eot) -- and one boost, finite and > 0. For a row of the device-side loop, h = the text tokens the row has sampled in this window since its last non-text
 * token (any sampled id >= eot empties it, so does the prompt step; wh_decode_greedy starts with it empty and does not count firstTokens). Before the softmax of each
 * step, logits[ row ][ t ] += boost, once, for every t such that u . t is a prefix of a phrase for some suffix u of h, the empty one included. -inf stays -inf:
 * suppressed tokens and the timestamp rules win. The order is vocabulary product -> suppress -> timestamp rules -> boost -> sampler, whatever the sampler; the
 * window's first sample is boosted too. Probabilities a run reports are the boosted distribution's. Not boosted: wh_decode, wh_lang_detect, wh_score_tokens,
 * wh_align_tokens, the beam step.
 * tokens: HOST [count][nMax], row p holds lens[ p ] ids; duplicates collapse. count == 0 turns it off (the state of every new context). Limits: 1024 phrases, 16
 * tokens each, 262144 table entries, a vocabulary of at most 65536 -- WH_E_INVALIDARG names the one violated, as for an id outside [0, eot), a boost that is not
 * finite or not > 0, a hypothesis-group context and WH_FLAG_PARITY_EXACT (wh_context_set_flags in turn refuses that flag while a set is held).
 * The tables (2.1 MB, sized for the limits) and maxSeq int32 states are allocated by the first non-empty call and never again; the tables and the boost live in
 * device memory and the captured step graphs are keyed on "a set is held" only. The call waits for the stream. */
WH_API int wh_context_set_boost( wh_context* c, const int32_t* tokens, const int32_t* lens, int count, int nMax, float boost );
/* Host only, no device needed: the automaton's tables for a set (the arguments and limits of wh_context_set_boost; nVocab <= 65536), as int32:
 * [0] nodes, [1] entries, [2] the boost's bits, [3] 0, off [nodes + 1], tok [entries], next [entries]. Node 0 is the root; node n owns entries off[ n ] ..
 * off[ n + 1 ), ascending in tok. The root's entries are its children; a deeper node's are the children along its failure chain without the root's, the deeper node
 * winning. delta( n, t ) = n's entry, else the root's, else the root; the tokens offered at n are n's and the root's. *nInts = the ints the tables take (0 for
 * count == 0); tables may be NULL to ask for it, cap = the ints it holds. */
WH_API int wh_boost_compile( const int32_t* tokens, const int32_t* lens, int count, int nMax, int tokenEot, int nVocab, float boost, int32_t* tables, int64_t cap,
	int64_t* nInts );
/* Host only: the twin of one step of the kernel on one row. state: a node or -1 (armed); reset as in wh_op_boost_logits. *newState and row [nVocab] in place.
 * Every call validates the whole of `tables` first, O( entries ): a twin for tests and tools, not a hot path. */
WH_API int wh_boost_step_host( const int32_t* tables, int64_t nInts, int32_t state, int32_t fed, int reset, float* row, int nVocab, int tokenEot, int32_t* newState );
/* No-repeat n-grams (Hugging Face generation's no_repeat_ngram_size, restricted to text columns): n = 0 off, 1 .. 8 on. With h[ 0, L ) the tokens a row has
 * sampled in the current window -- all of them, timestamps included, from the first sample behind the prompt -- the sample at position L finds -inf at every column
 * t < eot for which some i in [ 0, L - n ] has h[ i, i + n - 1 ) == h[ L - n + 1, L ) and h[ i + n - 1 ] == t: emitting t would complete an n-gram the window already
 * holds. With L < n nothing is masked; eot, the special ids and the timestamps are never masked, so a row always keeps mass and a window can always end; the prompt
 * (text carried over from the previous window included) does not count and no history survives into the next window. n = 1: no text token twice in a window.
 * The context keeps the history, n_text_ctx int32 per sequence, and a count per sequence in device memory. ONE small launch in front of the sampler appends the
 * token just fed -- the previous step's sample -- and masks the row; the prompt step of a window empties the histories and masks nothing. It applies to
 * wh_decode_greedy (the history starts at the call's first sample: firstTokens are not counted), wh_decode_window_start, _start_ragged and _continue, whatever the
 * sampler: greedy, wh_context_set_sampling, wh_context_set_sampling_rows. Unfiltered: wh_decode, wh_lang_detect, wh_align_tokens, wh_score_tokens and the beam step.
 * The buffers, for maxSeq sequences, are allocated by the first call that turns the option on and never again. n is an argument of the kernel and the captured step
 * graphs are keyed on it: a graph captured for one n never serves another, and a change of n captures again on the next window. The call waits for the stream: what
 * was queued runs under the n it was queued with. WH_E_INVALIDARG for n outside 0 .. 8, and to turn it on on a hypothesis-group context (the histories would have
 * to follow the beam's reorder) or under WH_FLAG_PARITY_EXACT (wh_context_set_flags in turn refuses that flag while the option is on). A context that never turns
 * it on launches, allocates and captures what it always did. */
WH_API int wh_context_set_no_repeat( wh_context* c, int n );
WH_API int wh_context_set_no_speech( wh_context* c, int on );
WH_API int wh_decode_window_no_speech( wh_context* c, float* out );

/* Per-kernel-class GPU timings, the counterpart of the reference's GpuProfiler / iContext::timingsPrint
 * (Whisper/Utils/GpuProfiler.h:21-188, Whisper/Whisper/ContextImpl.misc.cpp:170-182). hipEvent pairs around every launch
 * on the context's stream while enabled; flops / bytes are the algorithmic work of the launches. */
typedef struct wh_profile_entry
{
	char name[ 32 ];
	int64_t calls;
	double ms, flops, bytes;
} wh_profile_entry;
WH_API int wh_profile_enable( wh_context* c, int on );	/* resets the counters */
WH_API int wh_profile_read( wh_context* c, wh_profile_entry* out, int cap, int* count );

/* Test / parity access to internal state (the reference reaches these through its Tracing probe points,
 * Whisper/Whisper/WhisperContext.cpp:142-638). All outputs HOST FP32.
 *   what = "encode-out"  [batch][n_ctx][d]           (only valid right after wh_encode)
 *          "exp-table"   [0x5000]: the model's copy of the reference's table_exp_f16 (ggml.c:1375-1385), entry i = fp16( expf( -|fp16 bits i| ) )
 *          "cross-k" / "cross-v"   layer, [batch][n_ctx][d] token-major like the reference's kvCross
 *          "self-k" / "self-v"     layer, [sequences][rows][d]
 * and, captured under WH_FLAG_DEBUG_CAPTURE by the wh_encode / wh_decode call that follows the flag:
 *          "enc.temp1"      conv1 + bias + GELU, [batch][2*n_ctx][d] (time-major; the reference's tensor is [d][2*n_ctx])
 *          "enc.layer0.in"  conv2 + GELU + positional embedding = input of encoder layer 0, [batch][n_ctx][d]
 *          "enc-KQV"        encoder layer 0 attention output, [batch][n_ctx][d] (heads side by side)
 *          "dec-KQV" / "dec-KQV#2"   decoder layer 0 self / cross attention output of the last wh_decode, [rows][d]
 */
WH_API int wh_debug_read( wh_context* c, const char* what, int layer, int rows, float* dstHost, int64_t dstCapFloats );
/* Decode-step graphs the context has captured (instantiated) since it was created, of every kind of step. A recapture costs a blocking +2 to +7 ms and changes
 * no result, so only this count shows a retention rule that regressed. Host only. */
WH_API int wh_debug_step_captures( wh_context* c, int* count );

/* Development micro-benchmarks (tools/gemm_probe.py): kind 0 = chain of empty kernels (variant = workgroups), 2 = the same
 * replayed from a hipGraph, 1 = tiled GEMM tile-shape variant on an M x N x K problem. Returns milliseconds per iteration. */
/* Bit mask of kernel-variant switches (whisper_amd/csrc/kernels.h eTuning) for in-process A/B runs; contexts created
 * afterwards (and their captured graphs) use the new setting. */
WH_API int wh_debug_set_tuning( uint32_t mask );
/* Integer knobs beyond the 32 switches (whisper_amd/csrc/kernels.h struct Options: "dec_tile", "dec_depth", "dec_wide_rows", "dec_deep_rows", "vocab_decrows",
 * "enc_chunk", "self_fuse_max_rows", "self_nq", "self_wave_min_rows", "enc_exp", "enc_sched", "exact_enc_layers", "exact_alt_order", "gemm_mf16", "dec_lds", "dec_lds_ks", "dec_split", "cross_mfma", "vocab_lds", "beam_regs", "reorder_group", "gemm_big_min_rows", "resample_lds_phases", "score_chunk_rows", "score_regs"); also settable as WH_OPT_<NAME> in the environment at load.
 * Unknown names and values outside [-1, 2^24]: WH_E_INVALIDARG (the environment form: ignored with a line on stderr). The options are process-global and read without
 * synchronisation by every launch: set them BEFORE contexts are created, never while another thread runs one. */
WH_API int wh_debug_set_option( const char* name, int value );
/* The current value of an option (its compiled-in default until wh_debug_set_option or WH_OPT_<NAME> changes it). Host only: works without a device. */
WH_API int wh_debug_get_option( const char* name, int* value );
WH_API int wh_debug_probe( wh_context* c, int kind, int variant, int M, int N, int K, int iters, float* msPerIter );

/* ---- op-level entry points (replace the MlContext methods, Whisper/ML/MlContext.h:13-113). Device pointers. ---- */

/* MlContext::mulMat with an FP16 weight (ComputeShaders/mulMatTiled.hlsl, mulMatByRowTiled.hlsl):
 * out[m][n] = sum_k fp16(a[m][k]) * w[n][k] (+ bias[n]) (+ residual[m][n]); a: FP16 [M][K] (already rounded, which is
 * what ggml does at ggml.c:4588-4611), w: FP16 [N][K], out FP32 [M][N]. bias/residual may be NULL.
 * Scratch: the K-split shapes (32 < M <= 128, N <= 2048, K >= 2048) keep their partial tiles in a buffer the library owns, one per
 * (device, stream), allocated by the first such call on that stream and reused by every later one. Calls on different streams may
 * therefore run concurrently; calls on one stream are ordered by it. */
WH_API int wh_op_mul_mat( void* stream, const void* aF16, const void* wF16, const float* bias, const float* residual,
	float* out, int M, int N, int K );
/* mulMat + addRepeatGelu (ComputeShaders/addRepeatGelu.hlsl): out FP16 [M][N] = gelu16( acc + bias ) */
WH_API int wh_op_mul_mat_gelu( void* stream, const void* aF16, const void* wF16, const float* bias, void* outF16, int M, int N, int K );
/* MlContext::norm + fmaRepeat (norm.hlsl, fmaRepeat1.hlsl): out FP16 [rows][d] = fp16( norm(x) * w + b ) */
WH_API int wh_op_layer_norm( void* stream, const float* x, const float* w, const float* b, void* outF16, int rows, int d );
/* MlContext::flashAttention, unmasked (flashAttention.hlsl:76-169 == ggml.c:5912-6097).
 * q, k: FP16 [batch*heads][nCtx][64]. vFrag: FP16 [batch*heads][64 * nCtxPad], nCtxPad = roundup(nCtx, 256), zero beyond
 * nCtx, in the operand order of the P.V matrix instruction (what the QKV product's epilogue writes):
 *   index(key, dd) = (((key>>4)*2 + (dd>>5))*64 + ((key>>2)&1)*32 + (dd&31))*8 + ((key>>3)&1)*4 + (key&3)
 * out: FP16 [batch][nCtx][heads*64]. */
WH_API int wh_op_flash_attention( void* stream, const void* q, const void* k, const void* vFrag, void* out, int batch, int heads, int nCtx );
/* Decoder attention of WhisperContext::decodeLayer (Whisper/Whisper/WhisperContext.cpp:455-470, 505-519: mulMat(K,Q) ->
 * diagMaskInf -> softMax -> mulMat(V,.)) on caches laid out [block][head][keyStride][64] FP16. q, out: FP16
 * [sequences*nTok][heads*64], q already scaled. causal: query i of a sequence sees keys <= nPast + i. `group` consecutive
 * sequences share one cache block (cross-attention of a window's hypotheses); parityThreads > 0 emulates the CPU path's
 * FP16 thread-partitioned P.V (ggml.c:4689-4735). */
WH_API int wh_op_decoder_attention( void* stream, const void* qF16, const void* kCache, const void* vCache, void* outF16, int sequences, int heads,
	int nTok, int nKeys, int keyStride, int causal, int nPast, int group, int parityThreads );
/* The cross-attention half of a decode step in one launch (WhisperContext.cpp:489-519): q = fp16( ( Wq . fp16( LayerNorm(x)
 * * lnW + lnB ) + qB ) * qScale ) per head inside the attention kernel; x: FP32 [sequences][heads*64]. */
WH_API int wh_op_decoder_cross_attention( void* stream, const float* x, const float* lnW, const float* lnB, const void* qW, const float* qB,
	float qScale, const void* kCache, const void* vCache, void* outF16, int sequences, int heads, int nKeys, int keyStride, int group );
/* softMax over rows with the reference's FP16 exp table semantics (softMax.hlsl / ggml.c:5030-5090): in place, FP32 */
WH_API int wh_op_soft_max( void* stream, float* x, int rows, int cols );

/* ---- op-level entry points of the encoder's fused products (what wh_encode builds by hand: conv1, conv2, Q/K/V, cross-K/V of every decoder layer) and of the
 * producer of conv1's operand. Device pointers; restated in numpy by tests/encoder_ops_ref.py. ---- */

/* The kernel family a product went to */
typedef enum wh_gemm_family
{
	WH_GEMM_TILED_128 = 0,	/* gemmTiled, a workgroup per 128 x 128 tile */
	WH_GEMM_TILED_256 = 1,	/* gemmTiled, a workgroup per 256 x 256 tile */
	WH_GEMM_TILED8 = 2,		/* gemmTiled8: persistent, 8 waves */
	WH_GEMM_TILED4 = 3		/* gemmTiled4: persistent, 4 waves */
} wh_gemm_family;
/* acc[m][n] = sum_k A(m)[k] * w[n][k] in FP32, then the epilogue `epi`. Row m of A starts at a + ( m / Mb ) * aBatchStride + ( m % Mb ) * lda and is K halves long
 * (rows may overlap: conv1 reads lda = n_mels apart); w: FP16 [N][K]. epi:
 *   0  out32[ o ] = ( acc + bias[n] ) + res[ o ], o = ( m / Mb ) * cBatchStride + ( m % Mb ) * ldc + n; bias, res may be NULL
 *   1  out16[ o ] = gelu16( acc + bias[n] ), the same o
 *   2  out32[ m * ldc + n ] = pe[ ( m % Mb ) * N + n ] + float( gelu16( acc + bias[n] ) )
 *   3  N = 3 * 64 * H, x = fp16( acc + bias[n] ), window b = m / T, t = m % T, column n = sel * 64 H + h * 64 + dd: sel 0 -> q, sel 1 -> k, both FP16 [b][h][T][64];
 *      sel 2 -> v, FP16 [b][h][64 * Tpad], at the index(t, dd) of wh_op_flash_attention. Nothing else of v is written.
 *   4  N = layers * 2 * 64 * H, column n = layer * 128 H + isV * 64 H + h * 64 + dd: k / v FP16 [layer][B][h][T][64] at window b = m / T; k = fp16( acc * scale ),
 *      v = fp16( acc + bias[n] ). Windows M / T .. B - 1 of every layer are not written (k and v may point at a later window of larger caches).
 * Checked here, since the launchers cannot see it: the operands the epilogue needs are non-NULL; M is whole segments of Mb rows (Mb >= M: one segment) and the
 * output segments do not overlap; ldc >= N; for epi 3 and 4 N as above, M % T == 0, and Tpad >= T a multiple of 16 (3) or B >= M / T (4). K a multiple of 64,
 * lda and aBatchStride multiples of 8. Otherwise WH_E_INVALIDARG and nothing is launched.
 * The product goes through the chooser wh_encode's products go through; *family (may be NULL) = the wh_gemm_family it chose under the tuning bits and options of
 * the moment, *wideEpi (may be NULL) = how the tiles leave: 0 column stores, 1 through LDS as 16-byte row stores, 2 = 1 with the lean epilogue on interior tiles. */
typedef struct wh_gemm_encoder_args
{
	const void* a;
	const void* w;
	const float* bias;
	const float* res;
	const float* pe;
	float* out32;
	void* out16;
	void* q;
	void* k;
	void* v;
	int64_t aBatchStride, cBatchStride;
	int32_t M, N, K, lda, Mb, ldc, epi, T, Tpad, H, B;
	float scale;
} wh_gemm_encoder_args;
WH_API int wh_op_gemm_encoder( void* stream, const wh_gemm_encoder_args* args, int32_t* family, int32_t* wideEpi );
/* The producer of conv1's operand: x16[ b * xBatchStride + ( t + 1 ) * nMels + c ] = fp16( mel_b[ c ][ off_b + t ] ) for t < rows, c < nMels, zero where
 * off_b + t is at or beyond the spectrogram's length; rows 0 and rows + 1 of every window (conv1's padding) are not written. Either offsetsHost (HOST int32 [batch],
 * NULL = all 0) with mel_b = melDev + b * melStride, FP32 [nMels][melLen]; or windowsHost (HOST [batch], what wh_encode_windows takes; a window with a NULL
 * melDev is silence). Offsets are >= 0, lengths > 0, xBatchStride >= ( rows + 2 ) * nMels, or WH_E_INVALIDARG. The call waits for the stream. */
WH_API int wh_op_mel_to_conv_input( void* stream, const float* melDev, int64_t melStride, int64_t melLen, const int32_t* offsetsHost, const wh_mel_window* windowsHost,
	void* x16, int64_t xBatchStride, int nMels, int rows, int batch );

/* ---- op-level entry points of the single-token step's own kernels (what wh_decode launches for 1 .. 4 sequences, and the fused self-attention half of a
 * lock-step batch of 9 .. 32): WhisperContext.cpp:412-520. Device pointers; no prefetch hints; restated in float64 by tests/decode_step_ref.py. ---- */

/* gemvSmall: out[m][n] = epilogue( sum_k w[n][k] * x[m][k] ), w FP16 [N][K], 1 <= M <= 4 rows, K a multiple of 8 and at most 8192, FP32 accumulation.
 * pro: 0  x = aF16, FP16 [M][K];
 *      1  x = fp16( LayerNorm( lnX[m] ) * lnW + lnB ), lnX FP32 [M][K], K <= 2048;
 *      3  x[m][h*64 + j] = fp16( ( sum over the 8 splits, in order, of part[m][h][s][j] ) * float( 1 / sum over the splits of the double at part[m][h][s][64] ) ),
 *         part FP32 [M][K/64][8][68] as wh_op_cross_split leaves it, K a multiple of 64.
 * epi: 0  out32 FP32 [M][N] = acc (+ bias[n]) (+ residual[m][n]);
 *      1  out16 FP16 [M][N] = gelu16( acc + bias[n] );
 *      2  the decoder's Q/K/V product (N = 3 K, K = 64 heads): qF16 FP16 [M][K] = fp16( ( acc + bias ) * scale ); row pos of sequence m of kCache / vCache,
 *         FP16 [M][heads][textCtx][64], = fp16( acc * scale ) / fp16( acc + bias ), pos = nPastDev ? nPastDev[ m ] : nPast. Nothing else in the caches is written.
 * Operands a combination does not use may be NULL. Bad shapes or missing operands: an error, nothing is launched. */
WH_API int wh_op_gemv_small( void* stream, int M, int N, int K, int epi, int pro, const void* wF16, const void* aF16, const float* lnX, const float* lnW,
	const float* lnB, const float* part, const float* bias, const float* residual, float* out32, void* out16, void* qF16, void* kCache, void* vCache, int heads,
	int textCtx, int nPast, const int32_t* nPastDev, float scale );
/* crossScores then crossSoftmaxPV: the cross-attention of up to 4 sequences over 8 key ranges per head, range length ( ( nKeys + 7 ) / 8 + 3 ) & ~3. The query is
 * wh_op_decoder_cross_attention's. scores FP32 [sequences][heads][keyStride] = K . q for key < nKeys; splitMax FP32 [sequences][heads][8] = the maximum of each
 * range (-inf for an empty one); part FP32 [sequences][heads][8][68]: 64 sums of exp16( score - max over ALL ranges ) * V, the double sum of the exponentials at
 * floats 64 .. 65, two floats never written. nKeys <= 1536, heads * 64 <= 1280. wh_op_gemv_small( pro 3 ) combines the ranges. */
WH_API int wh_op_cross_split( void* stream, const float* x, const float* lnW, const float* lnB, const void* qW, const float* qB, float qScale,
	const void* kCache, const void* vCache, float* scores, float* splitMax, float* part, int sequences, int heads, int nKeys, int keyStride );
/* selfBlockDec: LayerNorm -> this head's rows of the fused FP16 [3d][d] weight (query, key, value; bqkv FP32 [3d]) -> q = fp16( ( . + b ) * scale ),
 * k = fp16( . * scale ), v = fp16( . + b ) -> k, v stored at row pos of the sequence's caches, FP16 [sequences][heads][keyStride][64] -> causal attention over
 * rows 0 .. pos -> outF16 FP16 [sequences][d]. pos = nPastDev ? nPastDev[ sequence ] : nPast, in [0, keyStride); keyStride <= 512, d <= 1280. The sequences per
 * workgroup follow the option "self_nq", the projection unit the tuning bit TUNE_SELF_MFMA. */
WH_API int wh_op_self_block_dec( void* stream, const float* x, const float* lnW, const float* lnB, const void* wqkv, const float* bqkv, float scale,
	void* kCache, void* vCache, void* outF16, int sequences, int heads, int keyStride, int nPast, const int32_t* nPastDev );

/* ---- op-level entry points of the beam step's kernels (the routes wh_decode and wh_beam_window_* take). Device pointers. ---- */

/* The decoder's vocabulary softmax (same semantics as wh_op_soft_max), out of place: probs [rows][cols] = softmax( logits [rows][cols] ).
 * Takes the kernel the option "beam_regs" selects (the row in registers up to 52224 columns, the three-pass kernel beyond). */
WH_API int wh_op_vocab_soft_max( void* stream, const float* logits, float* probs, int rows, int cols );
/* The kernel of wh_context_set_suppress outside a context: logits[ row ][ ids[ i ] ] = -inf for every row and i < count, in place; every other float keeps its
 * bits. ids: DEVICE int32 [count]; an id outside [0, nVocab) is skipped. count == 0 launches nothing (ids may be NULL). Plain stores: no atomics, no LDS. */
WH_API int wh_op_suppress_logits( void* stream, float* logits, int rows, int nVocab, const int32_t* ids, int count );
/* One step of the kernel of wh_context_set_timestamp_rules outside a context, on logits [rows][nVocab] in place. recordsDev: DEVICE int32 [rows][4] = { last token
 * was a timestamp, the one before it was, the last timestamp id (0 = none), tokens sampled (negative = armed) }. reset 0: fedTokensDev [rows] (DEVICE; the token
 * each row sampled last) is folded into the row's record -- an armed record folds nothing and becomes the empty history -- and the ranges the rules give become
 * -inf; every other float keeps its bits. reset 1: every record becomes the empty history; 2: armed; neither touches the logits, fedTokensDev may be NULL.
 * 0 <= tokenEot < tokenBeg < nVocab and tokenBeg >= 1, or WH_E_INVALIDARG. Plain stores: no atomics, no LDS. */
WH_API int wh_op_timestamp_rules( void* stream, float* logits, int rows, int nVocab, int tokenEot, int tokenBeg, const int32_t* fedTokensDev, int reset, int32_t* recordsDev );
/* One step of the kernel of wh_context_set_boost outside a context, on logits [rows][nVocab] in place. tablesDev: DEVICE int32 [tableInts], what wh_boost_compile
 * wrote. statesDev: DEVICE int32 [rows], the node each row's history stands on (0 = the root, -1 = armed). reset 0: statesDev[ row ] moves over fedTokensDev[ row ]
 * (DEVICE; the token each row sampled last) -- an armed state, or a fed id outside [0, tokenEot), gives the root; reset 1: every state becomes the root; 2: armed,
 * fedTokensDev may be NULL. Then, in all three, the boost is added once to every token the new state offers (an armed state offers what the root does); every other
 * float keeps its bits. Plain loads and stores: no atomics, no LDS; every index read from device memory is held inside its buffer. */
WH_API int wh_op_boost_logits( void* stream, float* logits, int rows, int nVocab, int tokenEot, const int32_t* tablesDev, int64_t tableInts, const int32_t* fedTokensDev,
	int reset, int32_t* statesDev );
/* One step of the kernel of wh_context_set_no_repeat outside a context, on logits [rows][nVocab] in place. historyDev: DEVICE int32 [rows][cap], the tokens each row
 * has sampled; countsDev: DEVICE int32 [rows], how many of them (-1 = armed). reset 0: fedDev[ row ] (DEVICE; the token each row sampled last) is appended to the
 * row's history -- an armed row appends nothing and becomes the empty history, a full one (count == cap) drops the token -- and every column t < tokenEot that would
 * complete an n-gram the history holds becomes -inf; every other float keeps its bits. reset 1: every history becomes empty; 2: armed; neither touches the logits,
 * fedDev may be NULL. 1 <= n <= 8, 0 <= tokenEot <= nVocab, cap >= 1, or WH_E_INVALIDARG. Plain loads and stores: no atomics, no LDS; a count above cap or below
 * -1, history entries and fed ids outside the row are held inside their buffers. */
WH_API int wh_op_no_repeat_ngram( void* stream, float* logits, int rows, int nVocab, int tokenEot, int n, const int32_t* fedDev, int reset, int32_t* historyDev,
	int32_t* countsDev, int cap );
/* The language-detection kernel of wh_lang_detect on logits [rows][nVocab]: langP [rows][nLang] = the probabilities wh_op_vocab_soft_max gives at columns
 * tokenSot + 1 .. tokenSot + nLang, bit for bit, without writing the other columns; best [rows] = the index (0 .. nLang - 1) of the largest, exact ties
 * to the lower index. The row stays in registers: nVocab <= 52224; 1 <= nLang <= 1024 and the block inside the row, or WH_E_INVALIDARG. */
WH_API int wh_op_lang_probs( void* stream, const float* logits, int rows, int nVocab, int tokenSot, int nLang, float* langP, int32_t* best );
/* The kernel of wh_score_tokens outside a context: outDev[ r ] = the record (see wh_token_score) of row r of logits, rowStride >= nVocab floats apart, against
 * targetsDev[ r ]. One 1024-thread workgroup per row; the row is read once and kept in registers up to 52224 columns, read twice beyond (and everywhere with the
 * option "score_regs" 0): the same bits. The targets are downloaded and checked first, so the call waits for the stream: a target outside [0, nVocab),
 * rowStride < nVocab, a null pointer or rows < 1 is WH_E_INVALIDARG and nothing is launched. No atomics, no scratch memory. */
WH_API int wh_op_token_scores( void* stream, const float* logits, int64_t rowStride, int rows, int nVocab, const int32_t* targetsDev, wh_token_score* outDev );
/* wh_sample_best on probabilities [rows][nVocab]: out [rows]. tokenBeg .. nVocab - 1 are the timestamps; the specials are < tokenBeg. */
WH_API int wh_op_sample_best( void* stream, const float* probs, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot,
	int forceTimestamp, int isInitial, wh_token_data* out );
/* ---- temperature sampling (an extension: the reference has no temperature; the rules are DESIGN.md section 7 "Decoding fallback", restated in float64 by
 * tests/fallback_ref.py) ----
 * wh_op_vocab_soft_max_scaled: wh_op_vocab_soft_max of the FP32 array logits[ i ] * invT, each product rounded once to FP32 -- the bits of scaling on the host and
 *   calling wh_op_vocab_soft_max; the same choice of kernel (the row in registers up to 52224 columns, three passes beyond).
 * wh_op_sample_draw: one categorical draw per row of probs [rows][nVocab] under wh_op_sample_best's rules. tsEnd, sumTs, the best text token and onlyTs are that
 *   kernel's, on the probs given. The allowed set A: with onlyTs the columns [tokenBeg, tsEnd); otherwise every column < tokenBeg except sot / solm / not, plus
 *   [tokenBeg, tsEnd). u = ( ( (u64)x0 << 21 ) | ( x1 >> 11 ) ) * 2^-53, x = Philox4x32-10 with key ( seed & 0xffffffff, seed >> 32 ) at counter
 *   ( positionsDev[ row ], row, nonce, 0 ). W = the FP64 sum of p over A; the token is the first c in A whose FP64 prefix sum over A exceeds u W; if rounding
 *   leaves none, the last c in A with p[ c ] > 0; if W == 0, wh_op_sample_best's pick. out[ row ]: id, p = probs[ id ], and tid / pt / ptsum with the bits
 *   wh_op_sample_best gives on the row. The sums are formed tile by tile (64 columns) and scanned: an FP64 sum of at most 52 k non-negative terms moves by less
 *   than 5.8e-12 relative with its order, so a draw can differ from another summation order's only where u W lies that close to a prefix boundary.
 *   nVocab <= 65536; positionsDev: DEVICE int32 [rows]. No atomics, no scratch memory.
 * wh_op_philox_u: the u of each row, uOut DEVICE double [rows]. */
WH_API int wh_op_vocab_soft_max_scaled( void* stream, const float* logits, float invT, float* probs, int rows, int cols );
WH_API int wh_op_sample_draw( void* stream, const float* probs, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot,
	int forceTimestamp, int isInitial, uint64_t seed, uint32_t nonce, const int32_t* positionsDev, wh_token_data* out );
/* The per-row step of wh_context_set_sampling_rows outside a context: probsOut [rows][nVocab] (device) = the table softmax of logits * ( 1 / T_row ) (factor 1
 * for a greedy row), out[ row ] (device) = wh_op_sample_best's record of a greedy row, wh_op_sample_draw's record of a sampled row run on that row alone with
 * its seed and nonce. rowParams: HOST [rows]. The call waits for the stream. */
typedef struct wh_sample_row
{
	float temperature;	/* 0 = greedy, else (0, 4] */
	uint32_t nonce;
	uint64_t seed;
} wh_sample_row;
WH_API int wh_op_sample_rows( void* stream, const float* logits, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot,
	int forceTimestamp, int isInitial, const wh_sample_row* rowParams, const int32_t* positionsDev, float* probsOut, wh_token_data* out );
WH_API int wh_op_philox_u( void* stream, uint64_t seed, uint32_t nonce, int rows, const int32_t* positionsDev, double* uOut );
/* wh_beam_candidates on probabilities [rows][nVocab]: out [rows][width], width 1 .. 8. */
WH_API int wh_op_beam_candidates( void* stream, const float* probs, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot,
	int forceTimestamp, int isInitial, int width, wh_token_data* out );
/* The ranked beam step's self-attention cache reorder: sequence j continues sequence parents[ j ]. Caches FP16 [layers][maxSeq][heads][keyStride][64]
 * (cacheK, cacheV; scratchK / scratchV of the same size serve the two-phase copy); rowsDev[ j ] rows of sequence j move, clamped to [0, keyStride].
 * group > 1 with sequences % group == 0 and the option "reorder_group": the sequences of each group of `group` consecutive ones move in one launch
 * (rows = rowsDev of the group's first sequence; a parent outside its group leaves that sequence as it is); otherwise the two-phase copy.
 * Every parents[ j ] MUST lie in [0, sequences): the device reads them as they are. Bad sizes: WH_E_INVALIDARG. */
WH_API int wh_op_reorder_self_cache( void* stream, void* cacheK, void* cacheV, void* scratchK, void* scratchV, const int32_t* parents,
	const int32_t* rowsDev, int layers, int sequences, int maxSeq, int heads, int keyStride, int group );


/* ---- op-level entry points of token alignment (the kernels of wh_align_tokens). Device pointers. ---- */

/* The alignment matrix of `windows` windows. q: FP16 [layer - qLayer0][window][nMax][heads*64] (layers qLayerStride elements apart), the cross-attention query
 * rows, already scaled; kCache: FP16 [layer][window][heads][keyStride][64] (layers kLayerStride elements apart). headPairsDev: DEVICE int32 [nHeads][2] =
 * (layer, head), layer in [qLayer0, nLayers), in the order the heads are summed; rowsDev / keysDev: DEVICE int32 [windows], the rows (<= nMax <= 256) and keys
 * (<= min( keyMax, keyStride )) of each window. Per head: S = q k^T in FP32 on the matrix cores, softmax over the keys with FP32 exp, (P - mean) / std over the
 * window's rows per key column (FP64 sums in row order; std == 0 gives 0), median of 7 along the keys with reflect padding (none at 3 keys or fewer);
 * mDev: FP32 [windows][nMax][keyMax] = the mean over the heads, 0 outside a window's rows and keys. statsDev: scratch, FP32 [windows][nHeads][nMax][2].
 * No atomics and fixed summation orders: a window's bits do not depend on windows, its index or nMax. Indices read from device memory are clamped into the buffers. */
WH_API int wh_op_align_matrix( void* stream, const void* qF16, int64_t qLayerStride, int qLayer0, const void* kCache, int64_t kLayerStride, int nLayers, int heads,
	int keyStride, const int32_t* headPairsDev, int nHeads, const int32_t* rowsDev, const int32_t* keysDev, int windows, int nMax, int keyMax, float* statsDev, float* mDev );
/* Dynamic time warping in FP32, one workgroup per window. xDev: FP32 [windows][rowMax][keyMax] costs; rowsDev / keysDev: DEVICE int32 [windows], R <= rowMax <= 256 and
 * nKeys <= keyMax of each window, rowMax * ceil( keyMax / 16 ) * 4 <= 150 KB (the packed trace lives in LDS). cost[0][0] = 0, +inf elsewhere on the border;
 * cost[i][j] = x[i-1][j-1] + min( c0 = cost[i-1][j-1], c1 = cost[i-1][j], c2 = cost[i][j-1] ); trace 0 when c0 < c1 && c0 < c2, else 1 when c1 < c0 && c1 < c2, else 2;
 * row 0 of the trace is 2, column 0 is 1; walked back from ( R, nKeys ). framesDev: int32 [windows][rowMax], the smallest key index of the path inside each row
 * (a path cell in column 0 of the table counts as key 0), -1 for rows >= R; a window with R == 0 or nKeys == 0 is all -1. */
WH_API int wh_op_dtw( void* stream, const float* xDev, int windows, int rowMax, int keyMax, const int32_t* rowsDev, const int32_t* keysDev, int32_t* framesDev );
/* The kernel of wh_capture_append on device pointers: srcDev holds the chunk (`frames` sample frames, s16 or f32, 1 or 2 channels, aligned to its sample type),
 * n is the buffer position in front of it. Writes monoDev [n, n + frames), stereoDev (may be NULL: stereo not kept) [2 n, 2 ( n + frames )) and
 * featDev [( n + frames ) / 256 - n / 256][3]; reads monoDev [256 ( n / 256 ), n). WH_E_BOUNDS when n + frames > capSamples, WH_E_INVALIDARG for another format
 * or channel count, negative sizes, a null or misaligned pointer with frames > 0: nothing is launched. frames == 0 launches nothing and succeeds. */
WH_API int wh_op_capture_append( void* stream, const void* srcDev, int format, int channels, int64_t n, int64_t frames, int64_t capSamples, float* monoDev,
	float* stereoDev, float* featDev );
/* The kernel of wh_capture_append / wh_capture_flush on a stream at another rate, with every piece of the stream's state an argument: nIn input frames were
 * accepted before this chunk, frames below z read as zero (z moves only by a skip, so the outputs emitted so far are max( ready( nIn ), ceil( z L / M ) )), and
 * histReadDev holds stream frames [nIn - ( K - 1 ), nIn) of every filtered channel, [nf][K - 1] floats, nf = 3 for two channels with stereoDev, else 1 (frames
 * below max( 0, z ) are never read). Appends the outputs that become ready to monoDev / stereoDev at buffer position n, writes the features of the 256-sample
 * frames they complete to featDev and the history for nIn + frames to histWriteDev (another buffer than histReadDev); *nOutputs receives their number. flush != 0:
 * the end of the stream, frames == 0, srcDev and histWriteDev are not used. WH_E_BOUNDS when the outputs do not fit capSamples, WH_E_INVALIDARG for a rate outside
 * 1000 .. 384000 or 16000 itself, another format or channel count, negative sizes, z > nIn, a null or misaligned pointer: nothing is launched. */
WH_API int wh_op_capture_append_rate( void* stream, const void* srcDev, int format, int channels, int inRate, int64_t frames, int64_t nIn, int64_t z, int flush,
	const float* histReadDev, float* histWriteDev, int64_t n, int64_t capSamples, float* monoDev, float* stereoDev, float* featDev, int64_t* nOutputs );

#ifdef __cplusplus
}
#endif
#endif
