"""Python face of libWhisper.so, the COM-style host API (include/whisperApi.h) through its flat C mirror (include/whisper_c.h).

Mirrors how the reference's own callers drive it (Examples/main/main.cpp:174-330): loadModel -> createContext ->
fullDefaultParams -> runFull -> getResults. No fallback: without the shared libraries and a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "lib", "libWhisper.so")

# eFullParamsFlags (Whisper/API/sFullParams.h:21-35)
TRANSLATE, NO_CONTEXT, SINGLE_SEGMENT, PRINT_SPECIAL = 1, 2, 4, 8
TOKEN_TIMESTAMPS = 0x100
ALIGN_TOKENS = 0x1000      # extension: token times from the decoder's cross-attention by dynamic time warping (greedy runs of one stream)

CPP_EXPORTS = ["setupLogger", "loadModel", "initMediaFoundation", "findLanguageKeyW", "findLanguageKeyA", "getSupportedLanguages", "listGPUs"]
# extensions next to the seven names of whisper.def: one process per GPU, and K streams in lock step on one GPU
CPP_EXTENSIONS = ["loadModelShared", "createBatchRunner", "runFullBatch", "splitAtPauses", "setAlignmentHeads"]

_lib = None


class WhisperError(RuntimeError):
    def __init__(self, hr: int, what: str):
        super().__init__("%s failed: HRESULT 0x%08x" % (what, hr & 0xFFFFFFFF))
        self.hr = hr & 0xFFFFFFFF


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise RuntimeError("libWhisper.so is missing: run `python -m whisper_amd.build`")
        L = C.CDLL(HOST_LIB_PATH)
        vp = C.c_void_p
        L.whisperc_load_model.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
        L.whisperc_release.argtypes = [vp]
        L.whisperc_release.restype = None
        L.whisperc_create_context.argtypes = [vp, C.POINTER(vp)]
        L.whisperc_special_tokens.argtypes = [vp, C.POINTER(C.c_int32)]
        L.whisperc_token_string.argtypes = [vp, C.c_int]
        L.whisperc_token_string.restype = C.c_char_p
        L.whisperc_is_multilingual.argtypes = [vp]
        L.whisperc_tokenize.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.c_int]
        L.whisperc_run_full.argtypes = [vp, vp, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int, vp, C.c_int, C.c_int]
        L.whisperc_run_full_range.argtypes = [vp, vp, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int]
        L.whisperc_run_full_audio_ctx.argtypes = [vp, vp, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int, vp, C.c_int, C.c_int, C.c_int]
        L.whisperc_run_full_beam.argtypes = [vp, vp, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int, vp, C.c_int, C.c_int, C.c_int]
        L.whisperc_result_counts.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.whisperc_result_segment.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                              C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32]
        L.whisperc_run_full_tt.argtypes = [vp, vp, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int, vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int]
        L.whisperc_result_token_times.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
        L.whisperc_result_token.argtypes = [vp, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.whisperc_timings_print.argtypes = [vp]
        L.whisperc_run_streamed.argtypes = [vp, vp, C.c_uint64, C.c_char_p, C.c_uint32, C.c_int, vp, C.c_int, C.c_int,
                                            C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
        L.whisperc_batch_create.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.whisperc_batch_run.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, C.c_char_p, C.c_uint32, C.c_int, vp, C.c_int, C.c_int, vp, vp]
        L.whisperc_tr_counts.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.whisperc_tr_segment.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32]
        L.whisperc_tr_token.argtypes = [vp, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
        L.whisperc_detect_language.argtypes = [vp, vp, C.c_uint32, C.c_int32, vp, C.c_uint32, C.POINTER(C.c_int32)]
        L.whisperc_detected_language.argtypes = [vp, C.c_char_p, C.POINTER(C.c_float)]
        L.whisperc_debug_lang_probs.argtypes = [vp, C.c_int32, vp]
        L.whisperc_language_code.argtypes = [C.c_int32, C.c_char_p]
        L.whisperc_tr_language.argtypes = [vp, C.c_char_p, C.POINTER(C.c_float)]
        L.whisperc_debug_context_flags.argtypes = [vp, C.c_uint32, C.c_int32]
        L.whisperc_model_set_alignment_heads.argtypes = [vp, vp, C.c_int32]
        L.whisperc_set_fallback.argtypes = [vp, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint64]
        L.whisperc_window_stats.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
        L.whisperc_batch_set_fallback.argtypes = [vp, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint64]
        L.whisperc_tr_window_stats.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
        L.whisperc_non_speech_tokens.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
        L.whisperc_set_suppress_tokens.argtypes = [vp, vp, C.c_uint32]
        L.whisperc_batch_set_suppress_tokens.argtypes = [vp, vp, C.c_uint32]
        L.whisperc_set_boost_phrases.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_float]
        L.whisperc_batch_set_boost_phrases.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_float]
        L.whisperc_set_no_repeat_ngram.argtypes = [vp, C.c_int32]
        L.whisperc_batch_set_no_repeat_ngram.argtypes = [vp, C.c_int32]
        L.whisperc_phrase_spellings.argtypes = [vp, C.c_char_p, vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
        L.whisperc_debug_phrase_spellings.argtypes = [C.c_char_p, C.c_char_p, vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
        L.whisperc_set_timestamp_rules.argtypes = [vp, C.c_int32]
        L.whisperc_batch_set_timestamp_rules.argtypes = [vp, C.c_int32]
        L.whisperc_resample.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int64, C.POINTER(C.c_int64)]
        L.whisperc_load_audio.argtypes = [C.c_char_p, C.c_int32, vp, C.c_int64, C.POINTER(C.c_int64)]
        L.whisperc_run_full_stereo.argtypes = [vp, vp, vp, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int]
        L.whisperc_run_streamed_stereo.argtypes = [vp, vp, vp, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int, vp, C.c_int, C.c_int,
                                                   C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
        L.whisperc_batch_run_stereo.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, C.c_char_p, C.c_uint32, C.c_int, vp, C.c_int, C.c_int, vp, vp]
        L.whisperc_detect_speaker.argtypes = [vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint8)]
        L.whisperc_result_speakers.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
        L.whisperc_tr_speakers.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
        L.whisperc_sot_sequence.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32, vp, C.c_uint32, C.POINTER(C.c_uint32)]
        L.whisperc_score_tokens.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp]
        L.whisperc_batch_score.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp]
        L.whisperc_vad.argtypes = [vp, C.c_int64, vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.whisperc_plan_chunks.argtypes = [vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32, vp, vp, C.c_int32, C.POINTER(C.c_int32)]
        L.whisperc_debug_vad_decide.argtypes = [vp, C.c_int64, vp, C.POINTER(C.c_int64)]
        L.whisperc_set_speech_filter.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        L.whisperc_batch_set_speech_filter.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        L.whisperc_speech_spans.argtypes = [vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, vp, C.c_uint32, C.POINTER(C.c_uint32)]
        L.whisperc_result_speech_spans.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
        L.whisperc_tr_speech_spans.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
        L.whisperc_capture_create.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, C.POINTER(vp)]
        L.whisperc_capture_create_rate.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.whisperc_capture_write.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_uint32]
        L.whisperc_capture_close.argtypes = [vp]
        L.whisperc_capture_dropped.argtypes = [vp]
        L.whisperc_capture_dropped.restype = C.c_uint64
        L.whisperc_capture_destroy.argtypes = [vp]
        L.whisperc_capture_destroy.restype = None
        L.whisperc_run_capture.argtypes = [vp, vp, C.c_char_p, C.c_uint32, vp, vp, vp, vp]
        L.whisperc_run_capture_params.argtypes = [vp, vp, C.c_char_p, C.c_uint32, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
        _lib = L
    return _lib


N_LANGUAGES = 99


def language_codes() -> List[str]:
    """The codes of the 99 languages in id order (the language token of id i is sot + 1 + i)."""
    out = []
    buf = C.create_string_buffer(8)
    for i in range(N_LANGUAGES):
        _check(lib().whisperc_language_code(i, buf), "languageCode")
        out.append(buf.value.decode())
    return out


def finish_language_probs(p: np.ndarray):
    """The host half of language detection on its own (no device): (winner id, lang_probs) from the language tokens' probabilities --
    the reference's second softmax, exp( p ) / sum exp( p ) summed in descending order in single precision."""
    p = np.ascontiguousarray(p, np.float32)
    out = np.zeros(len(p), np.float32)
    best = lib().whisperc_debug_lang_probs(p.ctypes.data_as(C.c_void_p), len(p), out.ctypes.data_as(C.c_void_p))
    return best, out


def set_host_loop_rules(mode: int):
    """0 = the reference CPU model's whisper_full rules (default), 1 = its GPU model's ContextImpl rules."""
    _check(lib().whisperc_set_host_loop_rules(mode), "set_host_loop_rules")


def set_beam_ranking(on_host: bool):
    """eSamplingStrategy::BeamSearch: rank every step's candidates on the host (round 4's decoder, the checker) instead of on the device (default)."""
    _check(lib().whisperc_set_beam_ranking(1 if on_host else 0), "set_beam_ranking")


def _check(hr: int, what: str) -> int:
    if hr < 0:
        raise WhisperError(hr, what)
    return hr


PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32 = range(5)          # wh_pcm_format
_PCM_FORMATS = {"uint8": PCM_U8, "int16": PCM_S16, "int32": PCM_S32, "float32": PCM_F32}
SAMPLE_RATE = 16000


def resample(pcm: np.ndarray, rate: int, channel: int = -1) -> np.ndarray:
    """PCM at `rate` Hz -> mono float32 at 16 kHz, on the GPU (wh_resample_host: Kaiser-windowed sinc, FP64 sums). pcm: uint8 / int16 / int32 / float32,
    shape [n] or [n, C] with up to 8 channels; channel -1 = the mean of the channels, else that channel. rate 16000 converts and downmixes only."""
    pcm = np.ascontiguousarray(pcm)
    if pcm.dtype.name not in _PCM_FORMATS or pcm.ndim not in (1, 2):
        raise ValueError("resample: uint8, int16, int32 or float32 of shape [n] or [n, channels], not %s %s" % (pcm.dtype, pcm.shape))
    n, channels = pcm.shape[0], (pcm.shape[1] if pcm.ndim == 2 else 1)
    fmt = _PCM_FORMATS[pcm.dtype.name]
    n_out = C.c_int64()
    _check(lib().whisperc_resample(pcm.ctypes.data_as(C.c_void_p), fmt, channels, channel, rate, n, None, 0, C.byref(n_out)), "resample")
    out = np.empty(n_out.value, np.float32)
    _check(lib().whisperc_resample(pcm.ctypes.data_as(C.c_void_p), fmt, channels, channel, rate, n, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n_out)), "resample")
    return out


def load_audio(path: str, stereo: bool = False) -> np.ndarray:
    """iMediaFoundation::loadAudioFile: a WAV file of any rate, bit depth and channel count as 16 kHz float32 -- mono [n], or with stereo=True the first two
    channels [n, 2] (a mono file twice -- the iAudioBuffer of a mono file has no stereo data; this function copies its one channel)."""
    n = C.c_int64()
    _check(lib().whisperc_load_audio(path.encode(), int(stereo), None, 0, C.byref(n)), "loadAudioFile")
    out = np.empty((n.value, 2) if stereo else (n.value,), np.float32)
    _check(lib().whisperc_load_audio(path.encode(), int(stereo), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)), "loadAudioFile")
    return out


# eSpeakerChannel (iContext::detectSpeaker, Context.speakers): which channel of a stereo recording is louder during a segment
SPEAKER_UNSURE, SPEAKER_LEFT, SPEAKER_RIGHT, NO_STEREO_DATA = 0, 1, 2, 0xFF


def _stereo_at_16k(stereo, sample_rate: int, n_mono: int) -> np.ndarray:
    """The stereo PCM beside a run's mono PCM: [n, 2] float32 at 16 kHz; at another sample_rate each channel is resampled on the GPU like the mono.
    n must be the mono's length after resampling: the two are one recording."""
    stereo = np.asarray(stereo)
    if stereo.ndim != 2 or stereo.shape[1] != 2:
        raise ValueError("stereo: an array of shape [n, 2], not %s" % (stereo.shape,))
    if sample_rate == SAMPLE_RATE:
        stereo = np.ascontiguousarray(stereo, np.float32)
    else:
        if stereo.dtype.name not in _PCM_FORMATS:
            stereo = stereo.astype(np.float32)
        stereo = np.ascontiguousarray(np.stack([resample(stereo, sample_rate, channel=c) for c in range(2)], 1))
    if stereo.shape[0] != n_mono:
        raise ValueError("stereo: %d frames beside %d mono samples at 16 kHz" % (stereo.shape[0], n_mono))
    return stereo


def _speakers_of(call, h) -> List[int]:
    n = C.c_uint32()
    _check(call(h, None, 0, C.byref(n)), "speakers")
    out = np.zeros(n.value, np.uint8)
    if n.value:
        _check(call(h, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), "speakers")
    return [int(x) for x in out]


def _at_16k(pcm: np.ndarray, sample_rate: int) -> np.ndarray:
    """What the run entry points take: mono float32 at 16 kHz; another sample_rate is resampled on the GPU first."""
    pcm = np.asarray(pcm)
    if sample_rate == SAMPLE_RATE or pcm.dtype.name not in _PCM_FORMATS:
        pcm = np.ascontiguousarray(pcm, np.float32)       # float64 and the like: cast as the 16 kHz path always did
    return pcm if sample_rate == SAMPLE_RATE else resample(pcm, sample_rate)


VAD_FRAME = 256             # samples per voice-activity frame: 16 ms at 16 kHz


def vad(pcm: np.ndarray, sample_rate: int = 16000):
    """Voice activity of a mono recording: (speech uint8 [n // 256], last_speech). speech[f] = 1 where frame f = samples [256 f, 256 f + 256) at 16 kHz is
    speech; last_speech = the sample behind the last speech frame (0 = none). The features (energy, dominant frequency, spectral flatness: wh_vad_features)
    are computed on the GPU, the reference's decision loop (Moattar & Homayounpour 2009) runs on the host. Another sample_rate is resampled on the GPU first."""
    pcm = _at_16k(pcm, sample_rate)
    n, last = C.c_int64(), C.c_int64()
    _check(lib().whisperc_vad(pcm.ctypes.data_as(C.c_void_p), len(pcm), None, 0, C.byref(n), None), "vad")
    speech = np.zeros(n.value, np.uint8)
    _check(lib().whisperc_vad(pcm.ctypes.data_as(C.c_void_p), len(pcm), speech.ctypes.data_as(C.c_void_p), speech.size, C.byref(n), C.byref(last)), "vad")
    return speech, last.value


def vad_decide(features: np.ndarray):
    """The host half of vad() on its own (no device): (speech, last_speech) from float32 [n, 3] features = energy, F, SFM per frame."""
    feat = np.ascontiguousarray(features, np.float32).reshape(-1, 3)
    speech, last = np.zeros(len(feat), np.uint8), C.c_int64()
    _check(lib().whisperc_debug_vad_decide(feat.ctypes.data_as(C.c_void_p), len(feat), speech.ctypes.data_as(C.c_void_p), C.byref(last)), "vad_decide")
    return speech, last.value


def plan_chunks(pcm: np.ndarray, max_len: int = 480000, min_len: int = 240000, pause_frames: int = 21, sample_rate: int = 16000):
    """Where to cut a long mono recording into independent pieces for BatchRunner.run: [(first_sample, count_samples)] at 16 kHz, a partition of the
    recording into pieces of at most max_len and -- but for the last -- at least min_len samples, cut in the middle of pauses of at least pause_frames
    frames of 256 samples (vad()), or where 21 frames hold the least energy when a piece holds no pause (Whisper::splitAtPauses)."""
    pcm = _at_16k(pcm, sample_rate)
    n = C.c_int32()
    args = (pcm.ctypes.data_as(C.c_void_p), len(pcm), max_len, min_len, pause_frames)
    _check(lib().whisperc_plan_chunks(*args, None, None, 0, C.byref(n)), "plan_chunks")
    first, count = np.zeros(n.value, np.int64), np.zeros(n.value, np.int64)
    _check(lib().whisperc_plan_chunks(*args, first.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), "plan_chunks")
    return [(int(f), int(c)) for f, c in zip(first, count)]


def _speech_frames(min_silence, min_speech, pad):
    """seconds -> frames of 256 samples at 16 kHz, rounded; 0 stays 0 (the library's default of that parameter)"""
    return tuple(int(round(float(v) * SAMPLE_RATE / VAD_FRAME)) for v in (min_silence, min_speech, pad))


def _spans_of(call, *front) -> list:
    """a (..., int64 [cap][2] or NULL, cap, *count) entry point -> [(first_sample, end_sample)]"""
    n = C.c_uint32()
    _check(call(*front, None, 0, C.byref(n)), "speechSpans")
    out = np.zeros((n.value, 2), np.int64)
    if n.value:
        _check(call(*front, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), "speechSpans")
    return [(int(a), int(b)) for a, b in out]


def speech_spans(pcm: np.ndarray, min_silence: float = 2.0, min_speech: float = 0.256, pad: float = 0.4, sample_rate: int = 16000):
    """Whisper::speechSpans: where a mono recording holds speech, [(first_sample, end_sample)] at 16 kHz, ascending and disjoint -- what a run with
    Context.set_speech_filter of the same arguments transcribes. The detector's flags (vad()) are merged across gaps shorter than min_silence seconds, runs
    shorter than min_speech are dropped, and what is left is padded by `pad` on both sides. Seconds, rounded to frames of 256 samples. The defaults are
    faster-whisper's vad_filter values; nobody has measured them for this detector on real speech."""
    pcm = _at_16k(pcm, sample_rate)
    a, b, c = _speech_frames(min_silence, min_speech, pad)
    return _spans_of(lib().whisperc_speech_spans, pcm.ctypes.data_as(C.c_void_p), len(pcm), a, b, c)


CAPTURE_STEREO, CAPTURE_NO_DROP = 1, 2                      # eCaptureFlags
LISTENING, VOICE, TRANSCRIBING, STALLED = 1, 2, 4, 0x80     # eCaptureStatus bits
_SHOULD_CANCEL_T = C.CFUNCTYPE(C.c_int32, C.c_void_p)
_CAPTURE_STATUS_T = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_uint8)
_CAPTURE_PIECE_T = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int64)


class Capture:
    """iPcmCapture: a stream of PCM at sample_rate (1000 .. 384000 Hz; other rates than 16000 are resampled on the device chunk by chunk, with the file path's
    filter, and durations, start samples and times stay those of the 16 kHz stream) that the caller writes, from any thread, while Context.run_capture transcribes it on another. Durations in seconds
    (the reference's sCaptureParams). stereo: keep the two channels, so that Context.speakers() answers for every piece. no_drop: never discard samples when
    transcription falls behind -- the loop waits for the running piece, and write() blocks while more than max_duration + 1 s is queued and a loop is
    draining: for a source that is not real time."""

    def __init__(self, min_duration: float = 2.0, max_duration: float = 3.0, drop_start_silence: float = 0.25, pause_duration: float = 0.333,
                 stereo: bool = False, no_drop: bool = False, sample_rate: int = 16000):
        self.h = C.c_void_p()
        self.stereo, self.no_drop, self.sample_rate = stereo, no_drop, sample_rate
        if not 0 <= sample_rate < 2 ** 32:
            raise WhisperError(0x80070057, "createPcmCaptureAtRate")
        _check(lib().whisperc_capture_create_rate(min_duration, max_duration, drop_start_silence, pause_duration,
                                                  (CAPTURE_STEREO if stereo else 0) | (CAPTURE_NO_DROP if no_drop else 0), sample_rate, C.byref(self.h)), "createPcmCaptureAtRate")

    def write(self, samples: np.ndarray):
        """int16 or float32, [n] (mono) or [n, 2] (interleaved stereo); the dtype and the channel count of a capture do not change"""
        a = np.ascontiguousarray(samples)
        if a.dtype.name not in ("int16", "float32") or a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] != 2):
            raise ValueError("Capture.write: int16 or float32 of shape [n] or [n, 2]")
        _check(lib().whisperc_capture_write(self.h, a.ctypes.data_as(C.c_void_p), _PCM_FORMATS[a.dtype.name], 1 if a.ndim == 1 else 2, a.shape[0]), "iPcmCapture.write")

    def close(self):
        """the end of the stream: run_capture drains what is queued, transcribes what is left if it holds voice, and returns"""
        _check(lib().whisperc_capture_close(self.h), "iPcmCapture.close")

    def dropped_chunks(self) -> int:
        return int(lib().whisperc_capture_dropped(self.h))

    def release(self):
        if self.h:
            lib().whisperc_capture_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Model:
    """iModel."""

    def __init__(self, path: str, device: int = 0):
        self.h = C.c_void_p()
        _check(lib().whisperc_load_model(path.encode(), device, C.byref(self.h)), "loadModel")

    def close(self):
        if self.h:
            lib().whisperc_release(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def create_context(self) -> "Context":
        return Context(self)

    def create_batch_runner(self, max_slots: int = 0, groups: int = 0, greedy_chunk: int = 0, flags: int = 0) -> "BatchRunner":
        return BatchRunner(self, max_slots, groups, greedy_chunk, flags)

    def special_tokens(self):
        a = (C.c_int32 * 8)()
        _check(lib().whisperc_special_tokens(self.h, a), "getSpecialTokens")
        names = ("eot", "sot", "prev", "solm", "not_", "beg", "translate", "transcribe")
        return dict(zip(names, list(a)))

    def token_string(self, token: int) -> Optional[bytes]:
        return lib().whisperc_token_string(self.h, token)

    def is_multilingual(self) -> bool:
        return lib().whisperc_is_multilingual(self.h) == 0

    def sot_sequence(self, language: str = "en", translate: bool = False, timestamps: bool = False) -> List[int]:
        """Whisper::makeSotSequence: the tokens that select the task, as runFull builds them -- sot[, language, transcribe | translate], then the
        no-timestamps token unless `timestamps`."""
        out, n = (C.c_int32 * 8)(), C.c_uint32(0)
        _check(lib().whisperc_sot_sequence(self.h, language.encode(), int(translate), int(timestamps), out, 8, C.byref(n)), "makeSotSequence")
        return [int(out[i]) for i in range(n.value)]

    def set_alignment_heads(self, pairs: Sequence[Sequence[int]]):
        """Whisper::setAlignmentHeads: the (layer, head) pairs whose cross-attention weights ALIGN_TOKENS averages; [] restores the default (every head of
        the upper half of the decoder's layers)."""
        a = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        _check(lib().whisperc_model_set_alignment_heads(self.h, a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a)), "setAlignmentHeads")

    def non_speech_tokens(self) -> List[int]:
        """Whisper::getNonSpeechTokens: the ids openai-whisper suppresses by default (brackets, quotes that open a word, note symbols ...), found by exact match
        in this model's vocabulary; ascending."""
        n = C.c_uint32(0)
        _check(lib().whisperc_non_speech_tokens(self.h, None, 0, C.byref(n)), "getNonSpeechTokens")
        ids = np.zeros(max(n.value, 1), np.int32)
        _check(lib().whisperc_non_speech_tokens(self.h, ids.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), "getNonSpeechTokens")
        return [int(i) for i in ids[:n.value]]

    def phrase_spellings(self, text: str) -> List[List[int]]:
        """Whisper::phraseSpellings: one text phrase as token rows for set_boost_phrases -- the text as written and, when it does not begin with a space, the
        text behind one space (a word in mid-sentence); equal rows collapse. A spelling that is empty or longer than 16 tokens is an error naming the phrase."""
        tokens, lens, n = np.zeros((2, 16), np.int32), np.zeros(2, np.int32), C.c_uint32(0)
        _check(lib().whisperc_phrase_spellings(self.h, text.encode("utf-8"), tokens.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), 2, C.byref(n)), "phraseSpellings")
        return [[int(t) for t in tokens[r, :lens[r]]] for r in range(n.value)]

    def tokenize(self, text: str) -> List[int]:
        buf = (C.c_int32 * 4096)()
        n = _check(lib().whisperc_tokenize(self.h, text.encode(), buf, 4096), "tokenize")
        return list(buf[:n])


def _boost_rows(model: Model, phrases):
    """strings (each gives its spellings) or id lists | None -> ( int32 [count][nMax], int32 [count] ) for whisperc_set_boost_phrases"""
    rows: List[List[int]] = []
    for p in (phrases if phrases is not None else []):
        rows += model.phrase_spellings(p) if isinstance(p, str) else [[int(t) for t in p]]
    lens = np.array([len(r) for r in rows], np.int32)
    tokens = np.zeros((len(rows), max([1] + [len(r) for r in rows])), np.int32)
    for i, r in enumerate(rows):
        tokens[i, :len(r)] = r
    return tokens, lens


def _set_boost(fn, who: str, h, model: Model, phrases, boost):
    tokens, lens = _boost_rows(model, phrases)
    if len(lens) == 0:
        _check(fn(h, None, None, 0, 0, 0.0), who)
        return
    if boost is None:
        raise ValueError(who + ": a boost is required with phrases (there is no default)")
    _check(fn(h, tokens.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), len(lens), tokens.shape[1], float(boost)), who)


def _suppress_ids(model: Model, ids) -> np.ndarray:
    """ids | "non_speech" | None -> int32 array"""
    if ids is None:
        return np.zeros(0, np.int32)
    if isinstance(ids, str):
        if ids != "non_speech":
            raise ValueError('set_suppress_tokens: the only named set is "non_speech"')
        ids = model.non_speech_tokens()
    return np.ascontiguousarray(ids, np.int32).reshape(-1)


# sTokenScore of whisperApi.h: the record of Whisper::scoreTokens / scoreBatch (times in 100 ns ticks, zero unless aligned)
TOKEN_SCORE_DT = np.dtype([("logprob", "<f4"), ("best_logprob", "<f4"), ("best", "<i4"), ("rank", "<i4"), ("t0", "<u8"), ("t1", "<u8")])
SCORE_ALIGN = 1


def _score_request(model, tokens_or_text, language, translate, timestamps, prompt, align):
    """(prompt tokens, scored tokens) of a scoring request: text goes through the model's tokenize, the prompt is [prev + past text,] + the sot sequence"""
    tokens = model.tokenize(tokens_or_text) if isinstance(tokens_or_text, str) else [int(t) for t in tokens_or_text]
    seq = model.sot_sequence(language, translate, timestamps and not align)
    past = ([model.special_tokens()["prev"]] + [int(t) for t in prompt]) if prompt is not None and len(prompt) else []
    return np.ascontiguousarray(past + seq, np.int32), np.ascontiguousarray(tokens, np.int32)


def _score_dicts(model, tokens, recs, align):
    """The per-token dicts of Context.score / BatchRunner.score: the scored tokens and eot behind them"""
    ids = [int(t) for t in tokens] + [model.special_tokens()["eot"]]
    out = []
    for t, r in zip(ids, recs):
        d = dict(id=t, text=model.token_string(t), logprob=float(r["logprob"]), best=int(r["best"]), best_logprob=float(r["best_logprob"]), rank=int(r["rank"]))
        if align:
            d["t0"], d["t1"] = int(r["t0"]), int(r["t1"])
        out.append(d)
    total = float(np.sum(recs["logprob"].astype(np.float64)))
    return dict(tokens=out, sum_logprob=total, avg_logprob=total / len(out))


class WindowStatsC(C.Structure):
    """sWindowStats of whisperApi.h"""
    _fields_ = [("seek", C.c_int32), ("attempts", C.c_int32), ("temperature", C.c_float), ("noSpeech", C.c_float), ("avgLogprob", C.c_double),
                ("entropy", C.c_double), ("skipped", C.c_uint32), ("reserved", C.c_uint32)]


class Context:
    """iContext."""

    def __init__(self, model: Model):
        self.model = model
        self.h = C.c_void_p()
        _check(lib().whisperc_create_context(model.h, C.byref(self.h)), "createContext")

    def close(self):
        if self.h:
            lib().whisperc_release(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run_full(self, pcm: np.ndarray, language: str = "en", flags: int = 0, max_tokens: int = 0,
                 prompt: Optional[Sequence[int]] = None, n_max_text_ctx: int = -1, max_len: int = 0, thold_pt: float = 0.01,
                 thold_ptsum: float = 0.01, beam_width: int = 0, audio_ctx: int = 0, offset_ms: int = 0, duration_ms: int = 0, sample_rate: int = 16000,
                 stereo: Optional[np.ndarray] = None) -> int:
        """runFull on mono float32 16 kHz PCM (another sample_rate: PCM of any dtype resample() takes, resampled on the GPU first). Returns the HRESULT (0 = S_OK, 1 = S_FALSE: less than 1 s of audio). language "auto" (or ""): detected
        on the window at frame 0, whatever the run's offset (detected_language tells which).
        With TOKEN_TIMESTAMPS in flags the tokens of results() carry t0 / t1 / vlen and max_len > 0 wraps the segments.
        With ALIGN_TOKENS the token times come from the decoder's cross-attention by dynamic time warping instead (Model.set_alignment_heads chooses the heads);
        with both flags those times win. Not with beam_width (E_NOTIMPL).
        stereo: the recording's two channels, [n, 2] at the same sample_rate (what iAudioBuffer::getPcmStereo returns): speakers() then tells which channel
        is louder during each segment. Combines with offset_ms / duration_ms; not with beam_width, audio_ctx or TOKEN_TIMESTAMPS through this face."""
        pcm = _at_16k(pcm, sample_rate)
        pt = np.ascontiguousarray(prompt if prompt is not None else [], np.int32)
        if stereo is not None:
            if audio_ctx or beam_width > 0 or flags & TOKEN_TIMESTAMPS:
                raise ValueError("run_full: stereo does not combine with beam_width, audio_ctx or TOKEN_TIMESTAMPS")
            st = _stereo_at_16k(stereo, sample_rate, len(pcm))
            return _check(lib().whisperc_run_full_stereo(self.h, pcm.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p), len(pcm), language.encode(), flags,
                                                         max_tokens, pt.ctypes.data_as(C.c_void_p) if len(pt) else None, len(pt), n_max_text_ctx, offset_ms,
                                                         duration_ms), "runFull")
        if offset_ms or duration_ms:            # sFullParams::offset_ms / duration_ms: the range that is transcribed
            return _check(lib().whisperc_run_full_range(self.h, pcm.ctypes.data_as(C.c_void_p), len(pcm), language.encode(), flags, max_tokens,
                                                        pt.ctypes.data_as(C.c_void_p) if len(pt) else None, len(pt), n_max_text_ctx, offset_ms, duration_ms), "runFull")
        if audio_ctx:               # sFullParams::audio_ctx (ContextImpl.cpp:488-489)
            return _check(lib().whisperc_run_full_audio_ctx(self.h, pcm.ctypes.data_as(C.c_void_p), len(pcm), language.encode(), flags, max_tokens,
                                                            pt.ctypes.data_as(C.c_void_p) if len(pt) else None, len(pt), n_max_text_ctx, audio_ctx), "runFull")
        if beam_width > 0:          # eSamplingStrategy::BeamSearch with this beam_width (extension: the reference only declares it)
            return _check(lib().whisperc_run_full_beam(self.h, pcm.ctypes.data_as(C.c_void_p), len(pcm), language.encode(), flags, max_tokens,
                                                       pt.ctypes.data_as(C.c_void_p) if len(pt) else None, len(pt), n_max_text_ctx, beam_width), "runFull")
        if flags & (TOKEN_TIMESTAMPS | ALIGN_TOKENS):
            return _check(lib().whisperc_run_full_tt(self.h, pcm.ctypes.data_as(C.c_void_p), len(pcm), language.encode(), flags, max_tokens,
                                                     pt.ctypes.data_as(C.c_void_p) if len(pt) else None, len(pt), n_max_text_ctx,
                                                     thold_pt, thold_ptsum, max_len), "runFull")
        return _check(lib().whisperc_run_full(self.h, pcm.ctypes.data_as(C.c_void_p), len(pcm), language.encode(), flags, max_tokens,
                                              pt.ctypes.data_as(C.c_void_p) if len(pt) else None, len(pt), n_max_text_ctx), "runFull")

    def score(self, pcm: np.ndarray, tokens_or_text, language: str = "en", translate: bool = False, timestamps: bool = False,
              prompt: Optional[Sequence[int]] = None, align: bool = False, sample_rate: int = 16000):
        """Whisper::scoreTokens: how probable is this transcript for this clip (1 to 30 s of mono PCM; one window)? The tokens -- or the text, through the model's
        tokenize -- are fed to the decoder behind [prev + prompt,] sot, language, task[, no-timestamps], and each of them and the eot behind them is scored under
        the model's own distribution. Returns dict(tokens=[dict(id, text, logprob, best, best_logprob, rank[, t0, t1])], sum_logprob, avg_logprob).
        align: forced alignment of the known text -- t0 / t1 (100 ns ticks) from the decoder's cross-attention, as ALIGN_TOKENS gives a transcript of its own;
        text tokens only, and the prompt ends on the no-timestamps token whatever `timestamps` says."""
        pcm = _at_16k(pcm, sample_rate)
        pt, tk = _score_request(self.model, tokens_or_text, language, translate, timestamps, prompt, align)
        recs = np.zeros(len(tk) + 1, TOKEN_SCORE_DT)
        _check(lib().whisperc_score_tokens(self.h, pcm.ctypes.data_as(C.c_void_p), len(pcm), pt.ctypes.data_as(C.c_void_p), len(pt),
                                           tk.ctypes.data_as(C.c_void_p), len(tk), SCORE_ALIGN if align else 0, recs.ctypes.data_as(C.c_void_p)), "scoreTokens")
        return _score_dicts(self.model, tk, recs, align)

    def run_streamed(self, pcm: np.ndarray, language: str = "en", flags: int = 0, max_tokens: int = 0,
                     prompt: Optional[Sequence[int]] = None, n_max_text_ctx: int = -1, sample_rate: int = 16000, stereo: Optional[np.ndarray] = None):
        """iMediaFoundation::loadAudioFileData (the PCM wrapped as a float32 WAV image at sample_rate, which the loader resamples when it is not 16000) +
        iContext::runStreamed. Returns (HRESULT, [progress values the sink received]).
        stereo: as in run_full; the reader then holds the 16 kHz mono and stereo PCM (both resampled here when sample_rate is not 16000)."""
        pt = np.ascontiguousarray(prompt if prompt is not None else [], np.int32)
        prog = (C.c_double * 4096)()
        n = C.c_int()
        if stereo is not None:
            mono = _at_16k(pcm, sample_rate)
            st = _stereo_at_16k(stereo, sample_rate, len(mono))
            hr = _check(lib().whisperc_run_streamed_stereo(self.h, mono.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p), len(mono), language.encode(), flags,
                                                           max_tokens, pt.ctypes.data_as(C.c_void_p) if len(pt) else None, len(pt), n_max_text_ctx,
                                                           prog, 4096, C.byref(n)), "runStreamed")
            return hr, list(prog[:min(n.value, 4096)])
        wav = wav_bytes(pcm, sample_rate)
        hr = _check(lib().whisperc_run_streamed(self.h, wav, len(wav), language.encode(), flags, max_tokens,
                                                pt.ctypes.data_as(C.c_void_p) if len(pt) else None, len(pt), n_max_text_ctx,
                                                prog, 4096, C.byref(n)), "runStreamed")
        return hr, list(prog[:min(n.value, 4096)])

    def run_capture(self, capture: "Capture", on_piece=None, on_status=None, should_cancel=None, language: str = "en", flags: int = 0, max_tokens: int = 0,
                    prompt: Optional[Sequence[int]] = None, n_max_text_ctx: int = -1, beam_width: int = 0, audio_ctx: int = 0):
        """iContext::runCapture: the reference's capture loop over `capture` until it is closed and drained, or should_cancel() returns true. Every piece the
        loop fires -- at a pause once min_duration is buffered, or at max_duration -- is a run_full on a worker thread of the library with this context's
        decoding options; segment times are stream times. Returns the pieces as [(start_sample, n_samples, results)].
        on_piece(start_sample, n_samples, results) is called behind each piece, on the worker thread, while results() / speakers() of the context are that
        piece's; on_status(word) whenever a bit of LISTENING | VOICE | TRANSCRIBING | STALLED changes: on the calling thread, but for the fall of TRANSCRIBING
        of a capture without no_drop, which comes from the worker thread when the piece's job ends.
        language, flags, max_tokens, prompt, n_max_text_ctx, beam_width and audio_ctx are run_full's and hold for every piece. The other keywords of run_full
        belong elsewhere: stereo and sample_rate are the capture's, and a piece has no offset or duration of its own."""
        pt = np.ascontiguousarray(prompt if prompt is not None else [], np.int32)
        pieces = []
        errors = []

        def piece(_pv, start, n):
            try:
                res = self.results()
                pieces.append((int(start), int(n), res))
                if on_piece is not None:
                    on_piece(int(start), int(n), res)
            except BaseException as e:        # an exception cannot cross the C frames
                errors.append(e)

        def status(_pv, word):
            try:
                if on_status is not None:
                    on_status(int(word))
            except BaseException as e:
                errors.append(e)
            return 0

        def cancel(_pv):
            try:
                return 1 if (errors or (should_cancel is not None and should_cancel())) else 0
            except BaseException as e:
                errors.append(e)
                return 1

        cbs = (_SHOULD_CANCEL_T(cancel), _CAPTURE_STATUS_T(status), _CAPTURE_PIECE_T(piece))
        hr = lib().whisperc_run_capture_params(self.h, capture.h if capture is not None else None, language.encode(), flags, max_tokens,
                                               pt.ctypes.data_as(C.c_void_p) if len(pt) else None, len(pt), n_max_text_ctx, audio_ctx, beam_width,
                                               C.cast(cbs[0], C.c_void_p), C.cast(cbs[1], C.c_void_p), C.cast(cbs[2], C.c_void_p), None)
        if errors:
            raise errors[0]
        _check(hr, "runCapture")
        return pieces

    def detect_language(self, pcm: np.ndarray, offset_ms: int = 0, sample_rate: int = 16000):
        """whisper_lang_auto_detect on the 30 s window at offset_ms of mono float32 16 kHz PCM: (code, {code: p}). The p are the reference's
        lang_probs: a SECOND softmax over the language tokens' probabilities, so a clear winner reads ~0.02, not ~0.9; their order is what counts.
        Another sample_rate is resampled on the GPU first."""
        pcm = _at_16k(pcm, sample_rate)
        probs = np.zeros(N_LANGUAGES, np.float32)
        lang = C.c_int32(-1)
        _check(lib().whisperc_detect_language(self.h, pcm.ctypes.data_as(C.c_void_p), len(pcm), offset_ms, probs.ctypes.data_as(C.c_void_p), len(probs),
                                              C.byref(lang)), "detectLanguage")
        codes = language_codes()
        return codes[lang.value], {c: float(v) for c, v in zip(codes, probs)}

    def set_device_flags(self, flags: int, parity_threads: int = 1):
        """wh_context_set_flags on the device context behind this iContext (parity tests: binding.WH_FLAG_PARITY_EXACT)."""
        _check(lib().whisperc_debug_context_flags(self.h, flags, parity_threads), "setDeviceFlags")

    def set_fallback(self, temperature_inc: Optional[float] = 0.2, logprob_thold: float = -1.0, entropy_thold: float = 2.4, no_speech_thold: float = 0.6, seed: int = 0):
        """Whisper::setDecodingFallback. set_fallback() or set_fallback(temperature_inc=0.2, ...) turns the feature on for this context's later runs: a greedy
        window whose scores look bad (mean log-probability below logprob_thold, or more than 32 tokens whose ids have an entropy below entropy_thold, or no
        timestamp) is decoded again by sampling at temperature_inc, 2 temperature_inc ... 1.0, and a window the model calls silent
        (P(<|nospeech|>) > no_speech_thold and a mean log-probability below logprob_thold) is dropped. set_fallback(None) turns it off, the state of a new
        context: the transcript is then what it always was. Greedy decoding of one stream only (beam_width: E_NOTIMPL)."""
        if temperature_inc is None:
            _check(lib().whisperc_set_fallback(self.h, 0, 0.0, 0.0, 0.0, 0.0, 0), "setDecodingFallback")
            return
        _check(lib().whisperc_set_fallback(self.h, 1, float(temperature_inc), logprob_thold, entropy_thold, no_speech_thold, seed), "setDecodingFallback")

    def set_suppress_tokens(self, ids=None):
        """Whisper::setSuppressedTokens: the logits of these token ids (text tokens, each below eot) are -inf before the softmax in every later run of this
        context -- greedy, the fallback's sampled attempts, beam search -- so they are never emitted. "non_speech": Model.non_speech_tokens(). None or []
        turns it off, the state of a new context: the transcript is then what it always was."""
        a = _suppress_ids(self.model, ids)
        _check(lib().whisperc_set_suppress_tokens(self.h, a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a)), "setSuppressedTokens")

    def set_no_repeat_ngram(self, n: Optional[int]):
        """Whisper::setNoRepeatNgram (Hugging Face's no_repeat_ngram_size on text tokens): in every later run of this context -- greedy, and each sampled attempt
        of the fallback -- a text token that would complete an n-gram the window has already sampled is forbidden on the device. n = 1 .. 8; 0 or None turns it
        off, the state of a new context. There is no default n: none has been measured on a real checkpoint. With it on, beam search raises (E_NOTIMPL)."""
        _check(lib().whisperc_set_no_repeat_ngram(self.h, int(n or 0)), "setNoRepeatNgram")

    def set_boost_phrases(self, phrases=None, boost: Optional[float] = None):
        """Whisper::setBoostedPhrases ("hotwords"): in every later run of this context -- greedy, and each sampled attempt of the fallback -- `boost` is added to
        the logit of every token that continues one of `phrases` after what was just emitted. phrases: strings (Model.phrase_spellings gives each its two
        spellings) or lists of text-token ids. None or [] turns it off, the state of a new context. There is no default boost: none has been measured on a
        real checkpoint. Beam search with a set held is E_NOTIMPL."""
        _set_boost(lib().whisperc_set_boost_phrases, "setBoostedPhrases", self.h, self.model, phrases, boost)

    def set_speech_filter(self, min_silence: Optional[float] = 2.0, min_speech: float = 0.256, pad: float = 0.4):
        """Whisper::setSpeechFilter (faster-whisper's vad_filter, whisper.cpp's --vad): every later run_full / run_streamed of this context finds the speech on the
        device (speech_spans' rules, the same arguments in seconds), transcribes only that and reports every time -- segments, tokens under ALIGN_TOKENS -- on
        the recording's own clock; speakers() are answered on the original stereo PCM. speech_spans() then tells what the last run used. A recording without
        speech gives hr 0 and no segment. set_speech_filter(None) turns it off, the state of a new context: the run is then what it always was. With it on,
        offset_ms / duration_ms raise (E_INVALIDARG) and TOKEN_TIMESTAMPS raises (E_NOTIMPL); run_capture ignores it."""
        if min_silence is None:
            _check(lib().whisperc_set_speech_filter(self.h, 0, 0, 0, 0), "setSpeechFilter")
            return
        _check(lib().whisperc_set_speech_filter(self.h, 1, *_speech_frames(min_silence, min_speech, pad)), "setSpeechFilter")

    def speech_spans(self):
        """Whisper::getSpeechSpans: [(first_sample, end_sample)] the last run_full / run_streamed transcribed; empty with the filter off or without speech."""
        return _spans_of(lib().whisperc_result_speech_spans, self.h)

    def set_timestamp_rules(self, on: bool = True):
        """Whisper::setTimestampRules: every later run masks the logits on the device so that timestamps come in pairs, never go back in time within a window
        and close segments of non-zero length (openai-whisper's ApplyTimestampRules) -- greedy runs and the fallback's sampled attempts alike. Off, the state
        of a new context, the transcript is what it always was. With the rules on, beam search raises (E_NOTIMPL)."""
        _check(lib().whisperc_set_timestamp_rules(self.h, 1 if on else 0), "setTimestampRules")

    def window_stats(self):
        """What the fallback did with each window of the last run: [{seek, attempts, temperature, no_speech, avg_logprob, entropy, skipped}], empty when
        the feature was off."""
        return _window_stats_of(lib().whisperc_window_stats, self.h, "getWindowStats")

    @property
    def detected_language(self):
        """(code, p) of what the last run with language "auto" (or detect_language) on this context detected; None when nothing was detected."""
        code = C.create_string_buffer(8)
        p = C.c_float()
        hr = _check(lib().whisperc_detected_language(self.h, code, C.byref(p)), "detectedLanguage")
        return (code.value.decode(), p.value) if hr == 0 else None

    def results(self):
        """getResults(Tokens | Timestamps): list of segments {t0, t1 (100 ns ticks), text, tokens[{id, p, pt, ptsum}]}."""
        ns, nt = C.c_uint32(), C.c_uint32()
        _check(lib().whisperc_result_counts(self.h, C.byref(ns), C.byref(nt)), "getResults")
        out = []
        for i in range(ns.value):
            t0, t1, ft, ct = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
            text = C.create_string_buffer(4096)
            _check(lib().whisperc_result_segment(self.h, i, C.byref(t0), C.byref(t1), C.byref(ft), C.byref(ct), text, 4096), "getSegments")
            toks = []
            for j in range(ft.value, ft.value + ct.value):
                tid, p, pt, ps = C.c_int32(), C.c_float(), C.c_float(), C.c_float()
                _check(lib().whisperc_result_token(self.h, j, C.byref(tid), C.byref(p), C.byref(pt), C.byref(ps)), "getTokens")
                k0, k1, vl = C.c_uint64(), C.c_uint64(), C.c_float()
                _check(lib().whisperc_result_token_times(self.h, j, C.byref(k0), C.byref(k1), C.byref(vl)), "getTokens")
                toks.append(dict(id=tid.value, p=p.value, pt=pt.value, ptsum=ps.value, t0=k0.value, t1=k1.value, vlen=vl.value))
            out.append(dict(t0=t0.value, t1=t1.value, text=text.value, tokens=toks))
        return out

    def speakers(self) -> List[int]:
        """One eSpeakerChannel per segment of results(): what iContext::detectSpeaker answered for the segment's times when the segment was appended --
        SPEAKER_LEFT / SPEAKER_RIGHT where that channel's sum of |sample| is more than 1.1 times the other's, SPEAKER_UNSURE otherwise; NO_STEREO_DATA (0xFF)
        for every segment of a run without stereo data."""
        return _speakers_of(lib().whisperc_result_speakers, self.h)

    def detect_speaker(self, t0: int, t1: int) -> int:
        """iContext::detectSpeaker on the interval [t0, t1] (100 ns ticks). Like the reference's it answers only from the callbacks of a run, which this face
        does not have: here it raises WhisperError with OLE_E_BLANK (0x80040007). speakers() is how results carry the answer."""
        ch = C.c_uint8(NO_STEREO_DATA)
        _check(lib().whisperc_detect_speaker(self.h, t0, t1, C.byref(ch)), "detectSpeaker")
        return ch.value

    def timings_print(self):
        _check(lib().whisperc_timings_print(self.h), "timingsPrint")


def _window_stats_of(fn, h, what) -> list:
    """whisperc_window_stats / whisperc_tr_window_stats -> [{seek, attempts, temperature, no_speech, avg_logprob, entropy, skipped}]"""
    n = C.c_uint32()
    _check(fn(h, None, 0, C.byref(n)), what)
    if n.value == 0:
        return []
    arr = (WindowStatsC * n.value)()
    _check(fn(h, arr, n.value, C.byref(n)), what)
    return [dict(seek=w.seek, attempts=w.attempts, temperature=w.temperature, no_speech=w.noSpeech, avg_logprob=w.avgLogprob, entropy=w.entropy,
                 skipped=bool(w.skipped)) for w in arr]


def read_result(h) -> list:
    """iTranscribeResult -> list of segments {t0, t1 (100 ns ticks), text, tokens[{id, p, pt, ptsum, t0, t1, vlen}]}."""
    L = lib()
    ns, nt = C.c_uint32(), C.c_uint32()
    _check(L.whisperc_tr_counts(h, C.byref(ns), C.byref(nt)), "getSize")
    out = []
    for i in range(ns.value):
        t0, t1, ft, ct = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
        text = C.create_string_buffer(4096)
        _check(L.whisperc_tr_segment(h, i, C.byref(t0), C.byref(t1), C.byref(ft), C.byref(ct), text, 4096), "getSegments")
        toks = []
        for j in range(ft.value, ft.value + ct.value):
            tid, p, pt, ps = C.c_int32(), C.c_float(), C.c_float(), C.c_float()
            k0, k1, vl = C.c_uint64(), C.c_uint64(), C.c_float()
            _check(L.whisperc_tr_token(h, j, C.byref(tid), C.byref(p), C.byref(pt), C.byref(ps), C.byref(k0), C.byref(k1), C.byref(vl)), "getTokens")
            toks.append(dict(id=tid.value, p=p.value, pt=pt.value, ptsum=ps.value, t0=k0.value, t1=k1.value, vlen=vl.value))
        out.append(dict(t0=t0.value, t1=t1.value, text=text.value, tokens=toks))
    return out


class BatchRunner:
    """iBatchRunner (Whisper::createBatchRunner): K streams in lock step; each keeps the semantics of iContext::runFull."""

    def __init__(self, model: Model, max_slots: int = 0, groups: int = 0, greedy_chunk: int = 0, flags: int = 0):
        self.model = model
        self.h = C.c_void_p()
        _check(lib().whisperc_batch_create(model.h, max_slots, groups, greedy_chunk, flags, C.byref(self.h)), "createBatchRunner")

    def close(self):
        if self.h:
            lib().whisperc_release(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_fallback(self, temperature_inc: Optional[float] = 0.2, logprob_thold: float = -1.0, entropy_thold: float = 2.4, no_speech_thold: float = 0.6, seed: int = 0):
        """Whisper::setBatchDecodingFallback: Context.set_fallback's gates and temperature retries for every stream of this runner's later runs
        (set_fallback(None) turns them off, the state of a new runner). A window whose attempt fails stays in its slot and is decoded again in the next
        round at the next temperature -- one slot-round per retry -- while its neighbours move on; stream i draws under the key seed + i. After run /
        run_split, window_stats holds one list per stream (Context.window_stats' records; None for a stream without a result)."""
        if temperature_inc is None:
            _check(lib().whisperc_batch_set_fallback(self.h, 0, 0.0, 0.0, 0.0, 0.0, 0), "setBatchDecodingFallback")
            return
        _check(lib().whisperc_batch_set_fallback(self.h, 1, float(temperature_inc), logprob_thold, entropy_thold, no_speech_thold, seed), "setBatchDecodingFallback")

    def set_suppress_tokens(self, ids=None):
        """Whisper::setBatchSuppressedTokens: Context.set_suppress_tokens for every stream of this runner's later runs (one set for all of them)."""
        a = _suppress_ids(self.model, ids)
        _check(lib().whisperc_batch_set_suppress_tokens(self.h, a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a)), "setBatchSuppressedTokens")

    def set_no_repeat_ngram(self, n: Optional[int]):
        """Whisper::setBatchNoRepeatNgram: Context.set_no_repeat_ngram for every stream of this runner's later runs (one n for all of them)."""
        _check(lib().whisperc_batch_set_no_repeat_ngram(self.h, int(n or 0)), "setBatchNoRepeatNgram")

    def set_boost_phrases(self, phrases=None, boost: Optional[float] = None):
        """Whisper::setBatchBoostedPhrases: Context.set_boost_phrases for every stream of this runner's later runs (one set and one boost for all of them)."""
        _set_boost(lib().whisperc_batch_set_boost_phrases, "setBatchBoostedPhrases", self.h, self.model, phrases, boost)

    def set_speech_filter(self, min_silence: Optional[float] = 2.0, min_speech: float = 0.256, pad: float = 0.4):
        """Whisper::setBatchSpeechFilter: Context.set_speech_filter for every stream of this runner's later runs. Each stream is filtered when it is admitted
        and its times are mapped with its own map; a stream without speech gets an empty result with hr 0 and never takes a slot. After run / run_split,
        speech_spans holds one list per stream, relative to the stream's first sample (None for a stream without a result). None turns it off."""
        if min_silence is None:
            _check(lib().whisperc_batch_set_speech_filter(self.h, 0, 0, 0, 0), "setBatchSpeechFilter")
            return
        _check(lib().whisperc_batch_set_speech_filter(self.h, 1, *_speech_frames(min_silence, min_speech, pad)), "setBatchSpeechFilter")

    def set_timestamp_rules(self, on: bool = True):
        """Whisper::setBatchTimestampRules: Context.set_timestamp_rules for every stream of this runner's later runs (one switch for all of them)."""
        _check(lib().whisperc_batch_set_timestamp_rules(self.h, 1 if on else 0), "setBatchTimestampRules")

    def run(self, streams, language: str = "en", flags: int = 0, max_tokens: int = 0, prompt: Optional[Sequence[int]] = None,
            n_max_text_ctx: int = -1, want_results: bool = True, sample_rate: int = 16000, stereo: Optional[Sequence] = None):
        """streams: list of float32 PCM arrays (at 16 kHz; another sample_rate: every array is resampled on the GPU first, first_sample / count_samples then count
        16 kHz samples), or of (pcm, first_sample, count_samples) -- pieces of a recording share the array.
        Returns (HRESULT, [segments per stream or None], [per-stream HRESULT]). language "auto": every stream is detected on ITS OWN first window
        and transcribed in its own language; self.languages then holds (code, p) per stream (None where nothing was detected).
        stereo: per stream None or the [n, 2] stereo PCM of the stream's WHOLE array (pieces of a recording share it like the mono); self.speakers then
        holds one eSpeakerChannel per segment and stream (Context.speakers; NO_STEREO_DATA for a stream without stereo data, None without a result)."""
        n = len(streams)
        if stereo is not None and len(stereo) != n:
            raise ValueError("stereo: one entry (an array or None) per stream")
        st_ptrs, st_keep = (C.c_void_p * n)(), {}
        keep, ptrs, lens, first, cnt = [], (C.c_void_p * n)(), (C.c_uint32 * n)(), (C.c_int64 * n)(), (C.c_int64 * n)()
        resampled = {}              # id of a caller's array -> its 16 kHz version: the pieces of one recording keep sharing one buffer
        for i, s in enumerate(streams):
            pcm, f, c = (s, 0, 0) if not isinstance(s, tuple) else s
            if sample_rate != SAMPLE_RATE:
                if id(pcm) not in resampled:
                    resampled[id(pcm)] = resample(pcm, sample_rate)
                pcm = resampled[id(pcm)]
            assert pcm.dtype == np.float32 and pcm.flags["C_CONTIGUOUS"]
            keep.append(pcm)
            ptrs[i], lens[i], first[i], cnt[i] = pcm.ctypes.data, len(pcm), f, c
            if stereo is not None and stereo[i] is not None:
                if id(stereo[i]) not in st_keep:
                    st_keep[id(stereo[i])] = _stereo_at_16k(stereo[i], sample_rate, len(pcm))
                st_ptrs[i] = st_keep[id(stereo[i])].ctypes.data
        pt = np.ascontiguousarray(prompt if prompt is not None else [], np.int32)
        res = (C.c_void_p * n)()
        per = (C.c_int32 * n)()
        import time
        t0 = time.perf_counter()
        if stereo is None:
            hr = lib().whisperc_batch_run(self.h, n, ptrs, lens, first, cnt, language.encode(), flags, max_tokens,
                                          pt.ctypes.data_as(C.c_void_p) if len(pt) else None, len(pt), n_max_text_ctx, res, per)
        else:
            hr = lib().whisperc_batch_run_stereo(self.h, n, ptrs, st_ptrs, lens, first, cnt, language.encode(), flags, max_tokens,
                                                 pt.ctypes.data_as(C.c_void_p) if len(pt) else None, len(pt), n_max_text_ctx, res, per)
        self.last_run_seconds = time.perf_counter() - t0          # the library call alone (bench.py)
        out = []
        self.languages = []
        self.speakers = []
        self.window_stats = []
        self.speech_spans = []
        for i in range(n):
            out.append(read_result(res[i]) if (res[i] and want_results) else None)
            self.window_stats.append(_window_stats_of(lib().whisperc_tr_window_stats, res[i], "getResultWindowStats") if res[i] else None)
            self.speakers.append(_speakers_of(lib().whisperc_tr_speakers, res[i]) if (res[i] and want_results) else None)
            self.speech_spans.append(_spans_of(lib().whisperc_tr_speech_spans, res[i]) if res[i] else None)
            code, p = C.create_string_buffer(8), C.c_float()
            detected = bool(res[i]) and lib().whisperc_tr_language(res[i], code, C.byref(p)) == 0
            self.languages.append((code.value.decode(), p.value) if detected else None)
            if res[i]:
                lib().whisperc_release(res[i])
        _check(hr, "runFullBatch")
        return hr, out, [int(x) & 0xFFFFFFFF for x in per]


    def score(self, items, language: str = "en", translate: bool = False, timestamps: bool = False, prompt: Optional[Sequence[int]] = None):
        """Whisper::scoreBatch: Context.score for many (clip, transcript) pairs, up to the runner's max_slots per pass in the order given. items: a list of
        (pcm, tokens_or_text) or (pcm, first_sample, count_samples, tokens_or_text) -- float32 PCM at 16 kHz, pieces of a recording share the array.
        Returns (HRESULT of the first failure or 0, [Context.score's dict per item, None where the item failed], [per-item HRESULT]): an item that fails its
        checks does not keep its neighbours from being scored. Forced alignment is Context.score's."""
        n = len(items)
        keep, ptrs, lens, first, cnt = [], (C.c_void_p * n)(), (C.c_uint32 * n)(), (C.c_int64 * n)(), (C.c_int64 * n)()
        pps, pcs, tps, tcs, outs = (C.c_void_p * n)(), (C.c_uint32 * n)(), (C.c_void_p * n)(), (C.c_uint32 * n)(), (C.c_void_p * n)()
        for i, it in enumerate(items):
            pcm, f, c, what = (it[0], 0, 0, it[1]) if len(it) == 2 else it
            assert pcm.dtype == np.float32 and pcm.flags["C_CONTIGUOUS"]
            pt, tk = _score_request(self.model, what, language, translate, timestamps, prompt, False)
            recs = np.zeros(len(tk) + 1, TOKEN_SCORE_DT)
            keep.append((pcm, pt, tk, recs))
            ptrs[i], lens[i], first[i], cnt[i] = pcm.ctypes.data, len(pcm), f, c
            pps[i], pcs[i], tps[i], tcs[i], outs[i] = pt.ctypes.data, len(pt), tk.ctypes.data, len(tk), recs.ctypes.data
        per = (C.c_int32 * n)()
        hr = lib().whisperc_batch_score(self.h, n, ptrs, lens, first, cnt, pps, pcs, tps, tcs, 0, outs, per) & 0xFFFFFFFF
        res = [_score_dicts(self.model, k[2], k[3], False) if per[i] >= 0 else None for i, k in enumerate(keep)]
        return hr, res, [int(x) & 0xFFFFFFFF for x in per]

    def run_split(self, pcm: np.ndarray, flags: int = 0, sample_rate: int = 16000, **run_kwargs):
        """ONE long recording on the batched path: cut at pauses (plan_chunks), the pieces run as independent streams (NoContext is added to flags: a piece
        carries nothing over). Returns what run returns plus the plan: (HRESULT, [segments per piece or None], [per-piece HRESULT], [(first, count)]);
        segment times are relative to the recording. run_kwargs: run's language, max_tokens, prompt, n_max_text_ctx, want_results."""
        pcm = _at_16k(pcm, sample_rate)
        plan = plan_chunks(pcm)
        hr, out, per = self.run([(pcm, f, c) for f, c in plan], flags=flags | NO_CONTEXT, **run_kwargs)
        return hr, out, per, plan


def wav_bytes(pcm: np.ndarray, rate: int = 16000) -> bytes:
    """Mono float32 PCM -> the bytes of a RIFF/WAVE file (format 3 = IEEE float), what loadAudioFileData / openAudioFile read."""
    import struct
    data = np.ascontiguousarray(pcm, "<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 1, rate, rate * 4, 4, 32)
    return b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + \
        b"data" + struct.pack("<I", len(data)) + data
