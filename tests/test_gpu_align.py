"""GPU tests of token alignment (word-level timestamps from cross-attention): the DTW and matrix kernels at op level against tests/align_ref.py,
wh_align_tokens on a random-weight model after a real wh_encode, and the host library with the AlignTokens flag.

Tolerance of the matrix (DESIGN.md "Token alignment"): max |M - M_float64| <= 4 x max |M_float32 - M_float64|, both sides evaluated by align_ref on
the same FP16 q and k. The device sums its 64-term dot products and its softmax sums in another order than numpy's pairwise sums, each within a small
factor of them; the median is 1-Lipschitz and adds nothing. Both numbers are printed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from whisper_amd import binding, ggml_format as gf  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref as ar  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------------------------------
# wh_op_dtw
# ---------------------------------------------------------------------------------------------------------------------
def _op_dtw(xs, row_max=None, key_max=None):
    """xs: list of [R][nKeys] float32 matrices -> list of frames [R], from ONE call."""
    row_max = row_max or max(x.shape[0] for x in xs)
    key_max = key_max or max(x.shape[1] for x in xs)
    buf = np.full((len(xs), row_max, key_max), np.nan, np.float32)          # padding is never read: NaN would show
    for w, x in enumerate(xs):
        buf[w, :x.shape[0], :x.shape[1]] = x
    x_d = dev(buf)
    rows = dev(np.asarray([x.shape[0] for x in xs], np.int32))
    keys = dev(np.asarray([x.shape[1] for x in xs], np.int32))
    frames = torch.full((len(xs), row_max), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    binding.check(binding.lib().wh_op_dtw(None, ptr(x_d), len(xs), row_max, key_max, ptr(rows), ptr(keys), ptr(frames)))
    torch.cuda.synchronize()
    f = frames.cpu().numpy()
    for w, x in enumerate(xs):
        assert (f[w, x.shape[0]:] == -1).all()
    return [f[w, :x.shape[0]].copy() for w, x in enumerate(xs)]


DTW_SHAPES = [(1, 1), (1, 50), (2, 3), (64, 50), (65, 51), (228, 50), (256, 1500)]


@pytest.mark.parametrize("R,N", DTW_SHAPES)
def test_op_dtw_equals_the_numpy_dtw(R, N):
    x = np.random.default_rng(R * 2000 + N).standard_normal((R, N)).astype(np.float32)
    want = ar.dtw_fast(x)
    got = _op_dtw([x])[0]
    assert np.array_equal(got, want), (R, N, np.flatnonzero(got != want)[:8])
    assert (np.diff(got) >= 0).all()


def _tie_matrix(R, N, seed):
    return np.random.default_rng(seed).integers(-1, 2, (R, N)).astype(np.float32)


def _inf_matrix(R, N, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((R, N)).astype(np.float32)
    x[rng.random((R, N)) < 0.15] = np.inf
    x[R // 2, :] = np.inf                                  # a whole row of +inf: every path crosses it
    return x


def test_op_dtw_ties_infinities_and_a_ragged_batch():
    """Integer costs full of exact ties pin the trace rule; +inf cells (a whole row of them) must not produce NaN decisions; three windows of
    different shapes in one call equal the three single calls bit for bit."""
    ties = _tie_matrix(37, 61, 1)
    infs = _inf_matrix(23, 40, 2)
    plain = np.random.default_rng(3).standard_normal((64, 50)).astype(np.float32)
    singles = []
    for x in (ties, infs, plain):
        got = _op_dtw([x])[0]
        assert np.array_equal(got, ar.dtw_fast(x)), x.shape
        singles.append(got)
    assert np.array_equal(ar.dtw_fast(ties), ar.dtw(ties)[0])          # the vectorised reference is the plain loop
    batched = _op_dtw([ties, infs, plain])
    for a, b in zip(batched, singles):
        assert np.array_equal(a, b)
    # the same windows inside larger strides
    padded = _op_dtw([plain, ties, infs], row_max=100, key_max=77)
    for a, b in zip(padded, (singles[2], singles[0], singles[1])):
        assert np.array_equal(a, b)


def test_op_dtw_rejects_bad_sizes():
    L = binding.lib()
    x = torch.zeros(4, device="cuda")
    i = torch.ones(4, dtype=torch.int32, device="cuda")
    for windows, rows, keys in ((0, 1, 1), (1, 257, 1), (1, 0, 4), (1, 4, 0), (1, 256, 2500)):
        assert L.wh_op_dtw(None, ptr(x), windows, rows, keys, ptr(i), ptr(i), ptr(i)) == -1
    assert L.wh_op_dtw(None, None, 1, 1, 1, ptr(i), ptr(i), ptr(i)) == -1


# ---------------------------------------------------------------------------------------------------------------------
# wh_op_align_matrix
# ---------------------------------------------------------------------------------------------------------------------
HEADS_7 = [(0, 1), (0, 3), (0, 4), (1, 0), (1, 2), (1, 3), (1, 5)]      # skips heads, spans two layers
HEADS_1 = [(1, 2)]
N_LAYERS, N_HEADS = 2, 6


def _window(L, n_keys, seed, plant=True):
    """FP16 q [layers][L][H*64] and k [layers][n_keys][H*64] of one window, with a run of keys whose probabilities underflow to 0 in every row, for
    every head and in float64 too (q[., 0] = 30, k[planted, 0] = -30: S = -900 + noise). Returns q, k, the key that must come out as exactly 0."""
    rng = np.random.default_rng(seed)
    d = N_HEADS * 64
    q = (0.5 * rng.standard_normal((N_LAYERS, L, d))).astype(np.float16)
    k = (0.5 * rng.standard_normal((N_LAYERS, n_keys, d))).astype(np.float16)
    zero_key = None
    if plant:
        q[:, :, 0::64] = 30.0
        k[:, :, 0::64] = 0.0
        if n_keys <= 3:
            zero_key = n_keys - 1                            # unfiltered: the column itself
            k[:, zero_key, 0::64] = -30.0
        else:
            zero_key = n_keys // 2                           # the centre of 7 such columns: the median of 7 zeros
            k[:, zero_key - 3:zero_key + 4, 0::64] = -30.0
    return q, k, zero_key


def _op_align_matrix(windows, heads, q_layer0, n_max=None, key_stride=None, key_max=None):
    """windows: list of (q [layers][L][d], k [layers][n_keys][d]) -> list of M [L][n_keys] from ONE call. Padding rows and keys are NaN."""
    n_max = n_max or max(q.shape[1] for q, _ in windows)
    key_stride = key_stride or max(k.shape[1] for _, k in windows)
    key_max = key_max or key_stride
    W, d = len(windows), N_HEADS * 64
    nq = N_LAYERS - q_layer0
    qb = np.full((nq, W, n_max, d), np.nan, np.float16)
    kb = np.full((N_LAYERS, W, N_HEADS, key_stride, 64), np.nan, np.float16)
    for w, (q, k) in enumerate(windows):
        qb[:, w, :q.shape[1]] = q[q_layer0:]
        kb[:, w, :, :k.shape[1]] = k.reshape(N_LAYERS, k.shape[1], N_HEADS, 64).transpose(0, 2, 1, 3)
    q_d, k_d = dev(qb), dev(kb)
    heads_d = dev(np.asarray(heads, np.int32))
    rows = dev(np.asarray([q.shape[1] for q, _ in windows], np.int32))
    keys = dev(np.asarray([k.shape[1] for _, k in windows], np.int32))
    stats = torch.empty((W, len(heads), n_max, 2), dtype=torch.float32, device="cuda")
    M = torch.full((W, n_max, key_max), np.nan, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    binding.check(binding.lib().wh_op_align_matrix(None, ptr(q_d), W * n_max * d, q_layer0, ptr(k_d), W * N_HEADS * key_stride * 64, N_LAYERS, N_HEADS, key_stride,
                                                   ptr(heads_d), len(heads), ptr(rows), ptr(keys), W, n_max, key_max, ptr(stats), ptr(M)))
    torch.cuda.synchronize()
    m = M.cpu().numpy()
    out = []
    for w, (q, k) in enumerate(windows):
        L, n = q.shape[1], k.shape[1]
        assert (m[w, L:] == 0).all() and (m[w, :, n:] == 0).all()          # zero outside the window, every cell written
        out.append(m[w, :L, :n].copy())
    return out


_REF = {}


def _matrix_refs(L, n_keys, n_heads):
    """float64 and float32 evaluations of one case, computed once and shared."""
    key = (L, n_keys, n_heads)
    if key not in _REF:
        heads = HEADS_7 if n_heads == 7 else HEADS_1
        q, k, zero_key = _window(L, n_keys, 1000 * L + n_keys)
        m64 = ar.align_matrix(q, k, heads, L, n_keys, np.float64)
        m32 = ar.align_matrix(q, k, heads, L, n_keys, np.float32)
        _REF[key] = (q, k, zero_key, heads, m64, m32)
    return _REF[key]


@pytest.mark.parametrize("n_heads", [1, 7])
@pytest.mark.parametrize("n_keys", [3, 50, 51, 1500])
@pytest.mark.parametrize("L", [6, 65, 228])
def test_op_align_matrix_against_float64(L, n_keys, n_heads):
    q, k, zero_key, heads, m64, m32 = _matrix_refs(L, n_keys, n_heads)
    got = _op_align_matrix([(q, k)], heads, 1 if n_heads == 1 else 0)[0]
    assert np.isfinite(got).all()
    err = float(np.abs(got - m64).max())
    ref_err = float(np.abs(m32.astype(np.float64) - m64).max())
    print("align_matrix L=%d keys=%d heads=%d: max |device - float64| %.3e, max |float32 - float64| %.3e (bound 4 x = %.3e)" % (L, n_keys, n_heads, err, ref_err, 4 * ref_err))
    assert (m64[:, zero_key] == 0).all() and (got[:, zero_key] == 0).all()          # the planted column: finite and 0
    assert err <= 4.0 * ref_err, (err, ref_err)


def test_op_align_matrix_bits_do_not_depend_on_the_batch_or_the_padding():
    cases = [_matrix_refs(65, 51, 7), _matrix_refs(6, 50, 7), _matrix_refs(228, 3, 7)]
    alone = [_op_align_matrix([(c[0], c[1])], HEADS_7, 0)[0] for c in cases]
    batch = _op_align_matrix([(c[0], c[1]) for c in cases], HEADS_7, 0)
    padded = _op_align_matrix([(c[0], c[1]) for c in cases[::-1]], HEADS_7, 0, n_max=256, key_stride=100, key_max=90)[::-1]
    for a, b, p in zip(alone, batch, padded):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(a.view(np.uint32), p.view(np.uint32))


def test_op_align_matrix_rejects_bad_sizes():
    L = binding.lib()
    x = torch.zeros(64, device="cuda")
    i = torch.zeros(4, dtype=torch.int32, device="cuda")

    def call(n_heads=1, windows=1, n_max=4, key_max=4, q=x):
        return L.wh_op_align_matrix(None, ptr(q) if q is not None else None, 0, 0, ptr(x), 0, 1, 1, 4, ptr(i), n_heads, ptr(i), ptr(i), windows, n_max, key_max, ptr(x), ptr(x))
    assert call(n_heads=0) == -1 and call(windows=0) == -1 and call(n_max=257) == -1 and call(key_max=0) == -1 and call(q=None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# planted alignment, op level
# ---------------------------------------------------------------------------------------------------------------------
PLANTED_SEEDS = [11, 12, 13, 14, 15, 16]      # tried 11 .. 16 on the CPU (float64 and float32 both return the planted boundaries): none dropped
PLANTED_P = 3


def _planted(seed):
    """Keys in consecutive blocks of 5 .. 12 frames share a +-0.5 code per head, row p + r carries block r's code, noise 0.05."""
    rng = np.random.default_rng(seed)
    R = int(rng.integers(4, 12))
    lens = rng.integers(5, 13, R)
    bounds = np.concatenate([[0], np.cumsum(lens)])
    n_keys, L = int(bounds[-1]), PLANTED_P + R + 1
    d = N_HEADS * 64
    codes = rng.choice(np.array([-0.5, 0.5]), size=(N_LAYERS, R, d))
    q = 0.05 * rng.standard_normal((N_LAYERS, L, d))
    k = 0.05 * rng.standard_normal((N_LAYERS, n_keys, d))
    for r in range(R):
        q[:, PLANTED_P + r] += codes[:, r]
        k[:, bounds[r]:bounds[r + 1]] += codes[:, r][:, None, :]
    return q.astype(np.float16), k.astype(np.float16), bounds[:-1].astype(np.int32), L, n_keys, R


@pytest.mark.parametrize("seed", PLANTED_SEEDS)
def test_planted_alignment_is_recovered(seed):
    q, k, starts, L, n_keys, R = _planted(seed)
    for dt in (np.float64, np.float32):
        m = ar.align_matrix(q, k, HEADS_7, L, n_keys, dt)
        assert np.array_equal(ar.dtw(-m[PLANTED_P:L - 1].astype(np.float32))[0], starts), (seed, dt)
    m = _op_align_matrix([(q, k)], HEADS_7, 0)[0]
    got = _op_dtw([np.ascontiguousarray(-m[PLANTED_P:L - 1])])[0]
    assert np.array_equal(got, starts), (seed, got, starts)


# ---------------------------------------------------------------------------------------------------------------------
# wh_align_tokens
# ---------------------------------------------------------------------------------------------------------------------
def _pcm(seconds, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * 16000)) / 16000.0
    return (0.3 * np.sin(2 * np.pi * (200 + 40 * seed) * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.05 * rng.standard_normal(len(t))).astype(np.float32)


def _rows(sp, n_text, seed):
    rng = np.random.default_rng(seed)
    return [sp["sot"], sp["sot"] + 1, sp["transcribe"], sp["not_"]] + [int(x) for x in rng.integers(1000, 40000, n_text)] + [sp["eot"]]


def _check_window(ctx, hp, b, row, n_keys, frames, M, heads, bound_note):
    """One window of an align_tokens call against align_ref on the device's own q and k, and the numpy DTW on the device's own matrix."""
    L, p = len(row), 3
    layers = sorted({l for l, _ in heads})
    q = {l: ctx.debug_read("align-q", layer=l)[b].astype(np.float16) for l in layers}
    k = {l: ctx.debug_read("cross-k", layer=l)[b].astype(np.float16) for l in layers}
    m64 = ar.align_matrix(q, k, heads, L, n_keys, np.float64)
    m32 = ar.align_matrix(q, k, heads, L, n_keys, np.float32)
    got = M[b, :L, :n_keys]
    err, ref_err = float(np.abs(got - m64).max()), float(np.abs(m32.astype(np.float64) - m64).max())
    print("%s window %d (L=%d, keys=%d): max |device - float64| %.3e, max |float32 - float64| %.3e" % (bound_note, b, L, n_keys, err, ref_err))
    assert err <= 4.0 * ref_err, (err, ref_err)
    assert (M[b, L:] == 0).all() and (M[b, :, n_keys:] == 0).all()
    R = L - 1 - p
    want = ar.dtw_fast(np.ascontiguousarray(-got[p:L - 1]))
    assert np.array_equal(frames[b, :R], want) and (frames[b, R:] == -1).all()
    assert (np.diff(frames[b, :R]) >= 0).all() and frames[b, 0] >= 0 and frames[b, R - 1] < n_keys


def test_align_tokens_on_a_random_model():
    hp = gf.hparams_for("test-d128-ml")
    sp = gf.special_tokens(hp)
    model = binding.HipModel.from_ggml(gf.synth_model("test-d128-ml", seed=21, attn_sharpness=4.0))
    ctx = binding.HipContext(model, 3)
    mels = [ctx.mel_spectrogram(dev(_pcm(30, s))) for s in (1, 2, 3)]
    ctx.encode(torch.stack(mels))
    default_heads = [(l, h) for l in range(hp.n_text_layer // 2, hp.n_text_layer) for h in range(hp.n_text_head)]
    rows = [_rows(sp, 9, 1), _rows(sp, 60, 2), _rows(sp, 1, 3)]
    n_keys = [1500, 733, 50]

    # what a decode step gives when no alignment ran in between
    prompt = np.asarray([rows[0][:3]] * 3, np.int32)
    logits_before, _ = ctx.decode(prompt, 0)

    frames = ctx.align_tokens(rows, n_keys)
    M = ctx.debug_read("align-matrix")
    for b in range(3):
        _check_window(ctx, hp, b, rows[b], n_keys[b], frames, M, default_heads, "default heads")
    # a second call: the same bits. A window alone with nMax padding: held to its own query rows like the batch (the decoder pass picks its product
    # kernels by the total number of rows, so the FP16 query rows of a window move in their last bits with the batch; the alignment kernels do not:
    # test_op_align_matrix_bits_do_not_depend_on_the_batch_or_the_padding)
    frames2 = ctx.align_tokens(rows, n_keys)
    assert np.array_equal(frames, frames2) and np.array_equal(M.view(np.uint32), ctx.debug_read("align-matrix").view(np.uint32))
    f_alone = ctx.align_tokens(rows[:1], n_keys[:1], n_max=100)
    _check_window(ctx, hp, 0, rows[0], n_keys[0], f_alone, ctx.debug_read("align-matrix"), default_heads, "alone, nMax 100")
    frames = ctx.align_tokens(rows, n_keys)
    assert np.array_equal(frames, frames2)
    # decoding afterwards is what it is without the call
    logits_after, _ = ctx.decode(prompt, 0)
    assert np.array_equal(logits_before.view(np.uint32), logits_after.view(np.uint32))

    # one chosen head changes the matrix; count 0 restores the default
    model.set_alignment_heads([(1, 1)])
    f_one = ctx.align_tokens(rows, n_keys)
    M_one = ctx.debug_read("align-matrix")
    assert not np.array_equal(M_one, M)
    _check_window(ctx, hp, 1, rows[1], n_keys[1], f_one, M_one, [(1, 1)], "head (1, 1)")
    model.set_alignment_heads([])
    ctx.align_tokens(rows, n_keys)
    assert np.array_equal(M.view(np.uint32), ctx.debug_read("align-matrix").view(np.uint32))

    # refusals
    with pytest.raises(binding.WhisperHipError):
        model.set_alignment_heads([(hp.n_text_layer, 0)])
    with pytest.raises(binding.WhisperHipError):
        ctx.align_tokens([[sp["sot"], sp["not_"], sp["eot"]]], [100])             # no text token
    with pytest.raises(binding.WhisperHipError):
        ctx.align_tokens(rows[:1], [0])
    with pytest.raises(binding.WhisperHipError):
        ctx.align_tokens(rows[:1], [1501])
    ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 1)
    with pytest.raises(binding.WhisperHipError):
        ctx.align_tokens(rows[:1], n_keys[:1])
    ctx.set_flags(0)
    ctx.close()
    ctx5 = binding.HipContext(model, 1, hypotheses=5)
    ctx5.encode(mels[0])
    with pytest.raises(binding.WhisperHipError):
        ctx5.align_tokens(rows[:1], n_keys[:1])
    ctx5.close()
    model.close()


def test_align_tokens_honours_the_audio_context():
    hp = gf.hparams_for("test-d128-ml")
    sp = gf.special_tokens(hp)
    model = binding.HipModel.from_ggml(gf.synth_model("test-d128-ml", seed=22, attn_sharpness=4.0))
    ctx = binding.HipContext(model, 1)
    ctx.set_audio_ctx(512)
    ctx.encode(ctx.mel_spectrogram(dev(_pcm(12, 5))))
    rows = [_rows(sp, 17, 4)]
    with pytest.raises(binding.WhisperHipError):
        ctx.debug_read("align-matrix")                      # nothing has been aligned yet: WH_E_NOT_READY, not a stale buffer
    with pytest.raises(binding.WhisperHipError):
        ctx.align_tokens(rows, [513])
    with pytest.raises(binding.WhisperHipError):
        ctx.debug_read("align-q", layer=3)                  # a call that failed leaves nothing behind either
    frames = ctx.align_tokens(rows, [512])
    M = ctx.debug_read("align-matrix")                      # as wide as the context's audio context
    assert M.shape == (1, len(rows[0]), 512)
    got = M[0, :len(rows[0]), :512]
    want = ar.dtw_fast(np.ascontiguousarray(-got[3:len(rows[0]) - 1]))
    assert np.array_equal(frames[0, :len(want)], want)
    ctx.close()
    model.close()


# ---------------------------------------------------------------------------------------------------------------------
# the host library: iContext::runFull / runStreamed with AlignTokens, Model.set_alignment_heads, the refusals, whisper-main --align
# ---------------------------------------------------------------------------------------------------------------------
E_NOTIMPL = 0x80004001
TICKS = 100000          # 10 ms in the results' 100 ns ticks


def _strip(segs):
    return [(s["t0"], s["t1"], s["text"], [t["id"] for t in s["tokens"]]) for s in segs]


def _times(segs):
    return [[(t["t0"] // TICKS, t["t1"] // TICKS) for t in s["tokens"]] for s in segs]


def _library_pcm():
    t = np.arange(40 * 16000) / 16000.0
    rng = np.random.default_rng(7)
    return (0.25 * np.sin(2 * np.pi * 330 * t) * (1 + 0.6 * np.sin(2 * np.pi * 2.5 * t)) + 0.05 * rng.standard_normal(len(t))).astype(np.float32)


def _device_times(ggml_model, pcm, segs, sp, heads=None, streamed=False):
    """What wh_align_tokens gives for the windows of a run_full transcript of the conditioned layout (two segments per window, the next window seeks to
    the second one's end): (t0, t1) in 10 ms units per token, segment by segment. streamed: the windows as runStreamed makes them -- the spectrogram of
    frames [seek, min( seek + 3000, length )) alone, normalised on its own maximum (the previous one's when it ends where the previous request ended),
    encoded from its frame 0."""
    m = binding.HipModel.from_ggml(ggml_model)
    if heads:
        m.set_alignment_heads(heads)
    ctx = binding.HipContext(m, 1)
    pcm_dev = dev(pcm)
    mel = None if streamed else ctx.mel_spectrogram(pcm_dev)
    mel_len = len(pcm) // 160
    assert len(segs) % 2 == 0 and len(segs) >= 4
    out, seek, last_end = [], 0, -1
    for w in range(len(segs) // 2):
        pair = segs[2 * w:2 * w + 2]
        assert pair[0]["t0"] // TICKS >= seek
        ids = [t["id"] for s in pair for t in s["tokens"]]
        text = [t for t in ids if t < sp["eot"]]
        if streamed:
            i0, i1 = min(seek, mel_len), min(seek + 3000, mel_len)
            ctx.encode(ctx.mel_spectrogram_window(pcm_dev, i0, i1 - i0, reuse_previous_max=last_end == i1))
            last_end = i1
        else:
            ctx.encode(mel, offsets=[seek])
        n_keys = max(1, min(1500, (mel_len - seek) // 2))
        frames = ctx.align_tokens([[sp["sot"], sp["sot"] + 1, sp["transcribe"], sp["not_"]] + text + [sp["eot"]]], [n_keys])[0]
        k = 0
        for s in pair:
            n = sum(1 for t in s["tokens"] if t["id"] < sp["eot"])
            out.append(ar.token_times([t["id"] for t in s["tokens"]], frames[k:k + n + 1], seek, s["t0"] // TICKS, sp["beg"], sp["eot"]))
            k += n
        seek = pair[1]["t1"] // TICKS
    ctx.close()
    m.close()
    return out


def _check_monotone(segs, seg_times, sp):
    """t0 <= t1 for every token; text tokens never run backwards within a WINDOW (two segments of the conditioned layout), and some token has a duration."""
    assert len(segs) % 2 == 0
    for w in range(len(segs) // 2):
        prev = None
        for s, times in zip(segs[2 * w:2 * w + 2], seg_times[2 * w:2 * w + 2]):
            for t, (t0, t1) in zip(s["tokens"], times):
                assert t0 <= t1
                if t["id"] < sp["eot"]:
                    assert prev is None or t0 >= prev, (w, t0, prev)
                    prev = t1
    assert any(t1 > t0 for times in seg_times for (t0, t1) in times)


def test_library_align_tokens(tmp_path):
    from whisper_amd import api
    hp = gf.hparams_for("test-d128-ml")
    sp = gf.special_tokens(hp)
    ggml = gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=10)
    path = str(tmp_path / "cond.bin")
    gf.write_model(path, ggml)
    model = api.Model(path)
    ctx = model.create_context()
    pcm = _library_pcm()
    kw = dict(language="en", prompt=[1000], n_max_text_ctx=0)

    assert ctx.run_full(pcm, flags=api.NO_CONTEXT, **kw) == 0
    plain = ctx.results()
    assert len(plain) >= 4 and all(t["t0"] == 0 and t["t1"] == 0 for s in plain for t in s["tokens"])          # no token times without a flag
    assert ctx.run_full(pcm, flags=api.NO_CONTEXT | api.ALIGN_TOKENS, **kw) == 0
    aligned = ctx.results()
    assert _strip(aligned) == _strip(plain)                                       # ids, texts, segment times: untouched
    got = _times(aligned)
    want = _device_times(ggml, pcm, aligned, sp)
    assert got == want
    _check_monotone(aligned, got, sp)

    # chosen heads reach the run; an empty list restores the default
    model.set_alignment_heads([(3, 1)])
    assert ctx.run_full(pcm, flags=api.NO_CONTEXT | api.ALIGN_TOKENS, **kw) == 0
    one = ctx.results()
    assert _strip(one) == _strip(plain)
    assert _times(one) == _device_times(ggml, pcm, one, sp, heads=[(3, 1)])
    with pytest.raises(api.WhisperError):
        model.set_alignment_heads([(4, 0)])
    model.set_alignment_heads([])
    assert ctx.run_full(pcm, flags=api.NO_CONTEXT | api.ALIGN_TOKENS, **kw) == 0
    assert _times(ctx.results()) == got

    # max_len wraps on the aligned times
    assert ctx.run_full(pcm, flags=api.NO_CONTEXT | api.ALIGN_TOKENS, max_len=1, **kw) == 0
    wrapped = ctx.results()
    assert len(wrapped) > len(aligned) and [t["id"] for s in wrapped for t in s["tokens"]] == [t["id"] for s in aligned for t in s["tokens"]]
    assert [tt for s in _times(wrapped) for tt in s] == [tt for s in got for tt in s]

    # runStreamed takes the flag (it needs no PCM, unlike TokenTimestamps)
    hr, _ = ctx.run_streamed(pcm, flags=api.NO_CONTEXT, **kw)
    streamed_plain = ctx.results()
    hr2, _ = ctx.run_streamed(pcm, flags=api.NO_CONTEXT | api.ALIGN_TOKENS, **kw)
    streamed = ctx.results()
    assert hr == hr2 == 0 and _strip(streamed) == _strip(streamed_plain) and len(streamed) >= 4
    assert _times(streamed) == _device_times(ggml, pcm, streamed, sp, streamed=True)          # the streamed windows' own spectrograms, key counts and caches
    _check_monotone(streamed, _times(streamed), sp)

    # refusals: beam search and the batch runner
    with pytest.raises(api.WhisperError) as e:
        ctx.run_full(pcm, flags=api.NO_CONTEXT | api.ALIGN_TOKENS, beam_width=2, **kw)
    assert e.value.hr == E_NOTIMPL
    runner = model.create_batch_runner(max_slots=2)
    with pytest.raises(api.WhisperError) as e:
        runner.run([pcm], flags=api.NO_CONTEXT | api.ALIGN_TOKENS, **kw)
    assert e.value.hr == E_NOTIMPL
    runner.close()
    ctx.close()
    model.close()


def test_whisper_main_align(tmp_path):
    """whisper-main --align -ml 1 runs and writes the transcript of the run without it, cut at token boundaries; -h does not mention the option."""
    import subprocess
    import wave
    from whisper_amd import build
    hp = gf.hparams_for("test-d128-ml")
    path = str(tmp_path / "m.bin")
    gf.write_model(path, gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=10))
    wav = str(tmp_path / "a.wav")
    with wave.open(wav, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.clip(np.round(_library_pcm() * 32768.0), -32768, 32767).astype("<i2").tobytes())

    def run(*args):
        r = subprocess.run([build.CLI_BIN] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        return r.returncode, r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")

    rc, out, err = run("-m", path, "-f", wav, "--align", "-ml", "1")
    assert rc == 0 and len(out.strip().splitlines()) >= 4, err[-2000:]
    rc2, out2, err2 = run("-m", path, "-f", wav, "-ml", "1", "--align")          # anywhere on the command line
    assert rc2 == 0 and out2 == out
    rc3, plain, _ = run("-m", path, "-f", wav)
    assert rc3 == 0 and len(out.strip().splitlines()) > len(plain.strip().splitlines())
    h = run("-h")
    assert "--align" not in h[1] + h[2]
    assert run("--align", "-h")[1:] == h[1:]
