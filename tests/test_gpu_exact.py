"""WH_FLAG_PARITY_EXACT on the device: the reference CPU path's bits, and the timed kernels measured against them.

north_star asks for logits within 1e-3 of the reference CPU path. The reference is not one function: its decoder sums P.V in FP16 over
per-thread key ranges (Whisper/source/ggml.c:4689-4735), so its own logits move by 0.05 .. 0.5 with the thread count on random-weight models
and by >= 1.5e-3 however peaky the attention is made (tools/ref_band_sweep.py, profiles/r06_reference_band.txt). A tolerance of 1e-3 against
"the reference" is therefore only meaningful against the reference AT A GIVEN THREAD COUNT, computed in its own summation order -- which is what
the exact mode does (whisper_amd/csrc/exact.hip, primitives pinned on the CPU by tests/test_exact_cpu.py):

  1. exact mode == oracle/_ref, BIT FOR BIT: cross-attention caches of every decoder layer, self-attention caches, logits and probabilities, at 1 and
     at 3 threads (d = 128), and at the shape BASELINE measures (ggml-medium: 24 + 24 layers, d = 1024) at 1 and 16 threads.
  2. the timed path against the exact mode ON THE DEVICE at the medium and large-v2 shapes: the same windows, the same tokens; the difference is
     what the MFMA summation order, FP32 LayerNorm sums and the FP32 P.V product (more accurate than the reference's FP16 one) amount to.
"""
import os

import numpy as np
import pytest
import torch

from whisper_amd import binding
from whisper_amd import ggml_format as gf

pytestmark = pytest.mark.gpu


def _prompt(sp):
    return [sp["sot"], sp["sot"] + 1, sp["transcribe"]]


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32))


def test_exact_tables_are_the_reference_tables(ref_lib_available):
    """All 65536 entries of both tables ggml_init builds (ggml.c:1375-1385): built here on the host with the same expressions."""
    if not ref_lib_available:
        pytest.skip("oracle/_ref/libwhisper_ref.so not present")
    from oracle import ref
    g, e = ref.lookup_tables()
    model = gf.synth_model("test-d128", seed=1234, attn_sharpness=2.0)
    m = binding.HipModel.from_ggml(model)
    ctx = binding.HipContext(m, 1)
    assert np.array_equal(ctx.debug_read("exact-gelu-table"), g.view(np.float16).astype(np.float32), equal_nan=True)
    assert np.array_equal(ctx.debug_read("exact-exp-table"), e.view(np.float16).astype(np.float32), equal_nan=True)
    ctx.close()
    m.close()


def exact_against_the_reference(kind, model, tmp_path, n_threads, n_win, windows_checked, n_steps, layers=None):
    from oracle import ref
    import bench
    hp = model.hparams
    sp = gf.special_tokens(hp)
    path = str(tmp_path / (kind + ".bin"))
    gf.write_model(path, model)
    m = binding.HipModel.from_ggml(model)
    ctx = binding.HipContext(m, n_win)
    ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, n_threads)
    pcm = bench.synth_pcm(n_win, seed=100)
    pcm_dev = torch.from_numpy(pcm).cuda()
    mels = torch.stack([ctx.mel_spectrogram(pcm_dev[b]) for b in range(n_win)])
    ctx.encode(mels)
    layers = layers if layers is not None else range(hp.n_text_layer)
    gk = {il: ctx.debug_read("cross-k", il) for il in layers}
    gv = {il: ctx.debug_read("cross-v", il) for il in layers}
    toks = np.array([_prompt(sp)] * n_win, np.int32)
    steps = []
    n_past = 0
    for step in range(n_steps):
        gl, gp = ctx.decode(toks, n_past)
        steps.append((toks.copy(), n_past, gl.copy(), gp.copy()))
        n_past += toks.shape[1]
        toks = np.argmax(gl, axis=1).astype(np.int32).reshape(-1, 1)
    sk = ctx.debug_read("self-k", 0, n_past)
    sv = ctx.debug_read("self-v", hp.n_text_layer - 1, n_past)
    for b in windows_checked:
        w = ref.RefWhisper(path, n_threads=n_threads, log_level=0)
        w.set_mel_any(mels[b].cpu().numpy())
        w.encode(0)
        for il in layers:
            k, v = w.cross_kv(il)
            assert _bits_equal(gk[il][b], k), "%s window %d: cross-K of layer %d differs (max %g)" % (kind, b, il, np.abs(gk[il][b] - k).max())
            assert _bits_equal(gv[il][b], v), "%s window %d: cross-V of layer %d differs (max %g)" % (kind, b, il, np.abs(gv[il][b] - v).max())
        for step, (tk, npast, gl, gp) in enumerate(steps):
            rl, rp = w.decode([int(t) for t in tk[b]], npast)
            d = np.abs(gl[b] - rl[-1])
            print("%s, %d thread(s), window %d step %d: logits max |diff| %.3g, %d of %d differ" % (kind, n_threads, b, step, d.max(), int((d != 0).sum()), d.size))
            assert _bits_equal(gl[b], rl[-1]), "logits differ"
            assert _bits_equal(gp[b], rp[-1]), "probabilities differ"
        k0, _ = w.self_kv(0, n_past)
        _, v1 = w.self_kv(hp.n_text_layer - 1, n_past)
        assert _bits_equal(sk[b], k0) and _bits_equal(sv[b], v1), "self-attention caches differ"
        w.close()
    ctx.close()
    m.close()


@pytest.mark.parametrize("n_threads", [1, 3])
def test_exact_mode_is_the_reference_bit_for_bit(ref_lib_available, tmp_path, n_threads):
    """d = 128, three windows with different audio in one batch, windows 0 and 2 against the live reference: every cross-attention cache, the
    3-token prompt and 4 greedy steps, self-attention caches of the first and last layer. IDENTICAL, at 1 and at 3 threads."""
    if not ref_lib_available:
        pytest.skip("oracle/_ref/libwhisper_ref.so not present")
    model = gf.synth_model("test-d128", seed=1234, attn_sharpness=2.0)
    exact_against_the_reference("test-d128", model, tmp_path, n_threads, 3, (0, 2), 5)


def test_exact_mode_at_the_large_v3_shape(ref_lib_available, tmp_path):
    """128 mel bins (conv1's channels padded 128 -> 128: no padding chain) and the 51866-entry vocabulary."""
    if not ref_lib_available:
        pytest.skip("oracle/_ref/libwhisper_ref.so not present")
    model = gf.synth_model("test-d128-v3", seed=77, attn_sharpness=2.0)
    exact_against_the_reference("test-d128-v3", model, tmp_path, 2, 1, (0,), 3)


@pytest.mark.parametrize("n_threads", [1, 16])
def test_exact_mode_at_the_medium_shape(ref_lib_available, tmp_path, n_threads):
    """The shape BASELINE's metric is quoted on (ggml-medium: d = 1024, 16 heads, 24 + 24 layers, 51865 tokens): cross-attention caches of the first
    and last decoder layer bit-identical to the reference's (24 encoder layers upstream of them), the prompt and 3 steps bit-identical on logits and
    probabilities -- at 1 thread and at the 16 threads the other full-shape tests run the reference with."""
    if not ref_lib_available:
        pytest.skip("oracle/_ref/libwhisper_ref.so not present")
    model = gf.synth_model("medium", seed=1)
    exact_against_the_reference("medium", model, tmp_path, n_threads, 1, (0,), 4, layers=(0, model.hparams.n_text_layer - 1))


def _teacher_forced(ctx, mels, prompt, n_steps, enc_flags, dec_flags, tokens=None):
    ctx.set_flags(*enc_flags)
    ctx.encode(mels)
    ctx.set_flags(*dec_flags)
    out, fed = [], []
    toks, n_past = prompt, 0
    for st in range(n_steps + 1):
        gl, _ = ctx.decode(toks, n_past)
        out.append(gl.copy())
        fed.append(toks.copy())
        n_past += toks.shape[1]
        toks = tokens[st + 1] if tokens is not None and st + 1 < len(tokens) else np.argmax(gl, axis=1).astype(np.int32).reshape(-1, 1)
    ctx.set_flags(0, 1)
    return np.stack(out), fed


@pytest.mark.parametrize("kind,n_win,n_steps", [("medium", 4, 8), ("large-v2", 2, 4)])
def test_timed_path_against_the_exact_mode(kind, n_win, n_steps):
    """What north_star's "within 1e-3 on logits" can and cannot mean for the TIMED kernels, measured on the device at the shapes BASELINE names.

    Four runs of one context on the same windows, teacher-forced with the timed path's greedy tokens (3-token prompt + n_steps):
      T     the timed path (MFMA products, FP32 LayerNorm sums, FP32 P.V);
      E16   the exact mode at 16 threads  == the reference at 16 threads, bit for bit (the tests above);
      E0    the exact mode with the decoder's P.V rounded once per output: the value every thread count of the reference approximates;
      E0alt E0 with ONE change: the weight products add ggml_vec_dot_f16's 32 chains left to right instead of in ggml's tree -- the smallest
            re-ordering of the reference's own FP32 sums there is.
    Measured (profiles/r06_evidence/split_*.txt): |E0alt - E0| = 4.8e-3 max / 7.9e-4 mean at medium, 5.8e-3 / 9.6e-4 at large-v2 -- FP32 sums
    that differ in the last bit flip FP16 roundings of the activations (every product rounds its input to FP16, ggml.c:4588-4611), and 48 + 64
    layers carry that to the logits. So NO implementation that does not sum in exactly ggml's order can stay within 1e-3 in the max norm; the
    stated tolerance is meaningful in the MEAN (asserted below with the stated 1e-3 at the shape the metric is quoted on), and bit-exactly in
    the exact mode (asserted above: 0). The timed path is held to that floor: max and mean |T - E0| within 1.5 x of |E0alt - E0| measured in
    the same run, top-1 identical on every row, and T is no farther from the 16-thread reference than 2 x the reference's own distance to E0."""
    import bench
    model = gf.synth_model(kind, seed=1)
    hp = model.hparams
    sp = gf.special_tokens(hp)
    m = binding.HipModel.from_ggml(model)
    del model
    ctx = binding.HipContext(m, n_win)
    pcm_dev = torch.from_numpy(bench.synth_pcm(n_win, seed=100)).cuda()
    mels = torch.stack([ctx.mel_spectrogram(pcm_dev[b]) for b in range(n_win)])
    prompt = np.array([_prompt(sp)] * n_win, np.int32)
    X = binding.WH_FLAG_PARITY_EXACT
    T, fed = _teacher_forced(ctx, mels, prompt, n_steps, (0, 1), (0, 1))
    E16, _ = _teacher_forced(ctx, mels, prompt, n_steps, (X, 16), (X, 16), fed)
    E0, _ = _teacher_forced(ctx, mels, prompt, n_steps, (X, 0), (X, 0), fed)
    binding.set_option("exact_alt_order", 1)
    try:
        E0alt, _ = _teacher_forced(ctx, mels, prompt, n_steps, (X, 0), (X, 0), fed)
    finally:
        binding.set_option("exact_alt_order", 0)
    ctx.close()
    m.close()

    def dist(a, b):
        d = np.abs(a - b)
        return float(d.max()), float(d.mean())

    floor_max, floor_mean = dist(E0alt, E0)
    t_max, t_mean = dist(T, E0)
    r_max, r_mean = dist(E16, E0)
    t16_max, t16_mean = dist(T, E16)
    print("%s: re-ordered reference vs E0 %.2e / %.2e; timed vs E0 %.2e / %.2e; reference(16 threads) vs E0 %.2e / %.2e; timed vs reference(16) %.2e / %.2e (max / mean)"
          % (kind, floor_max, floor_mean, t_max, t_mean, r_max, r_mean, t16_max, t16_mean))
    assert floor_max > 1e-3, "the re-ordered reference stays within 1e-3: then the timed path must, too -- tighten this test"
    assert t_max <= 1.5 * floor_max and t_mean <= 1.5 * floor_mean
    if kind == "medium":
        assert t_mean <= 1e-3                      # north_star's tolerance, in the norm in which it can hold
    assert t16_max <= 2.0 * r_max + floor_max and t16_mean <= 2.0 * r_mean
    assert np.array_equal(T.argmax(-1), E0.argmax(-1)) and np.array_equal(T.argmax(-1), E16.argmax(-1))


_DEPTH_MODELS = {}


@pytest.fixture(scope="module")
def depth_model():
    """Two-layer synthetic models at the widths of large and tiny, built once per width for the cases below."""
    def get(d, heads):
        if d not in _DEPTH_MODELS:
            hp = gf.HParams(n_vocab=51865, n_audio_ctx=1500, n_audio_state=d, n_audio_head=heads, n_audio_layer=1,
                            n_text_ctx=448, n_text_state=d, n_text_head=heads, n_text_layer=2, n_mels=80, f16=1)
            _DEPTH_MODELS[d] = binding.HipModel.from_ggml(gf.synth_model(hp=hp, seed=21, attn_sharpness=2.0))
        return _DEPTH_MODELS[d]
    yield get
    for m in _DEPTH_MODELS.values():
        m.close()
    _DEPTH_MODELS.clear()


@pytest.mark.parametrize("d,heads,n_seq", [(1280, 20, 1), (1280, 20, 4), (1280, 20, 12), (1280, 20, 40), (384, 6, 1), (384, 6, 4), (384, 6, 12), (384, 6, 40)])
def test_single_token_steps_at_depth_against_the_exact_mode(depth_model, d, heads, n_seq):
    """The single-token kernels as wh_decode wires them, deep in the context: 1 and 4 sequences take decode1.hip (gemvSmall, the split cross-attention), 12 take
    selfBlockDec, 40 the separate self-attention launch. Every sequence has its own audio and its own prompt of P = 61, 125 and 443 tokens fed at n_past 0, then
    four single-token steps: they cross positions 64 and 128 (the ends of the score loops' 64-row passes) and end with 447 cached keys.
    Three runs of one context, teacher-forced with the timed run's tokens, as in test_timed_path_against_the_exact_mode: T the timed path, E0 the exact mode with
    P.V rounded once per output, E0alt the same with the smallest re-ordering of the reference's own FP32 sums. On the single-token steps max and mean |T - E0| stay
    within 1.5 x |E0alt - E0| measured in the same run, and the top token agrees wherever E0's margin over its runner-up exceeds twice that measured maximum."""
    import bench
    m = depth_model(d, heads)
    sp = gf.special_tokens(m.hp)
    ctx = binding.HipContext(m, n_seq)
    pcm_dev = torch.from_numpy(bench.synth_pcm(n_seq, seed=100 + n_seq)).cuda()
    mels = torch.stack([ctx.mel_spectrogram(pcm_dev[b]) for b in range(n_seq)])
    rng = np.random.default_rng(d + n_seq)
    lengths = (61, 125, 443)
    prompts = {P: rng.integers(0, sp["eot"], (n_seq, P)).astype(np.int32) for P in lengths}
    X = binding.WH_FLAG_PARITY_EXACT

    def run(flags, fed=None):
        ctx.set_flags(*flags)
        ctx.encode(mels)
        logits, tokens = {}, {}
        for P in lengths:
            toks, n_past = prompts[P], 0
            logits[P], tokens[P] = [], []
            for st in range(5):
                gl, _ = ctx.decode(toks, n_past)
                n_past += toks.shape[1]
                toks = fed[P][st] if fed is not None else np.argmax(gl, axis=1).astype(np.int32).reshape(-1, 1)
                tokens[P].append(toks)
                if st > 0:
                    logits[P].append(gl.copy())          # the four single-token steps
        ctx.set_flags(0, 1)
        return {P: np.stack(v) for P, v in logits.items()}, tokens

    T, fed = run((0, 1))
    E0, _ = run((X, 0), fed)
    binding.set_option("exact_alt_order", 1)
    try:
        E0alt, _ = run((X, 0), fed)
    finally:
        binding.set_option("exact_alt_order", 0)
    ctx.close()
    for P in lengths:
        floor, dist = np.abs(E0alt[P] - E0[P]), np.abs(T[P] - E0[P])
        print("d=%d, %d sequence(s), prompt %d: timed vs E0 max %.2e mean %.2e; re-ordered reference vs E0 max %.2e mean %.2e (bound 1.5 x)"
              % (d, n_seq, P, dist.max(), dist.mean(), floor.max(), floor.mean()))
        assert np.isfinite(T[P]).all()
        assert dist.max() <= 1.5 * floor.max() and dist.mean() <= 1.5 * floor.mean()
        top2 = np.sort(E0[P], axis=-1)[..., -2:]
        clear = (top2[..., 1] - top2[..., 0]) > 2.0 * floor.max()
        assert np.array_equal(T[P].argmax(-1)[clear], E0[P].argmax(-1)[clear])


def test_audio_ctx_override(ref_lib_available, tmp_path):
    """sFullParams::audio_ctx (Whisper/Whisper/ContextImpl.cpp:24, 55, 488-489 == whisper.cpp's exp_n_audio_ctx): the encoder runs on the first audio_ctx
    positions of a window, the decoder's cross-attention sees that many keys. wh_context_set_audio_ctx against the reference with the same override:
    the exact mode bit for bit (cross-attention cache of layer 0 -- the reference packs the layers at the overridden stride --, logits, probabilities), the timed
    path within the bounds of the d = 128 tests; then back to the full context on the same device context: identical to a fresh one (nothing of the short
    window survives in the padding rows the convolutions and the V operand rely on)."""
    if not ref_lib_available:
        pytest.skip("oracle/_ref/libwhisper_ref.so not present")
    from oracle import ref
    import bench
    model = gf.synth_model("test-d128", seed=1234, attn_sharpness=2.0)
    hp = model.hparams
    sp = gf.special_tokens(hp)
    path = str(tmp_path / "m.bin")
    gf.write_model(path, model)
    m = binding.HipModel.from_ggml(model)
    ctx = binding.HipContext(m, 2)
    pcm_dev = torch.from_numpy(bench.synth_pcm(2, seed=100)).cuda()
    mels = torch.stack([ctx.mel_spectrogram(pcm_dev[b]) for b in range(2)])
    toks = np.array([_prompt(sp)] * 2, np.int32)
    ctx.encode(mels)
    full_logits, _ = ctx.decode(toks, 0)
    # ascending first: the exact mode's encoder buffers are allocated by its first encode and must hold every audio_ctx that follows
    for n_ctx in (1, 700, 1):
        w = ref.RefWhisper(path, n_threads=2, log_level=0)
        w.set_mel_any(mels[1].cpu().numpy())
        w.set_audio_ctx(n_ctx)
        w.encode(0)
        rk, rv = w.cross_kv(0)
        rl, rp = w.decode([int(t) for t in toks[1]], 0)
        w.close()
        ctx.set_audio_ctx(n_ctx)
        ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)
        ctx.encode(mels)
        gk, gv = ctx.debug_read("cross-k", 0), ctx.debug_read("cross-v", 0)
        gl, gp = ctx.decode(toks, 0)
        n = n_ctx * hp.n_audio_state             # the device returns [windows][audio_ctx][d] packed at the front of the (full-size) host array
        assert _bits_equal(gk.reshape(-1)[n:2 * n], rk.reshape(-1)[:n]), "cross-K differs at audio_ctx %d" % n_ctx
        assert _bits_equal(gv.reshape(-1)[n:2 * n], rv.reshape(-1)[:n])
        assert _bits_equal(gl[1], rl[-1]) and _bits_equal(gp[1], rp[-1]), "logits differ at audio_ctx %d: max %g" % (n_ctx, np.abs(gl[1] - rl[-1]).max())
        ctx.set_flags(0, 1)
        ctx.encode(mels)
        tl, _ = ctx.decode(toks, 0)
        d = np.abs(tl[1] - rl[-1])
        print("audio_ctx %d: exact mode identical; timed path vs the reference (2 threads): max %.2e mean %.2e" % (n_ctx, d.max(), d.mean()))
        assert d.max() < 0.25 and d.mean() < 4e-2 and int(np.argmax(tl[1])) == int(np.argmax(rl[-1]))
    ctx.set_audio_ctx(0)
    ctx.encode(mels)
    again, _ = ctx.decode(toks, 0)
    assert np.array_equal(again, full_logits)
    ctx.close()
    m.close()


def test_timed_encoder_at_reduced_audio_ctx_against_the_exact_mode():
    """The encoder a context actually launches at a reduced audio_ctx, where its fused products sit on the other side of their epilogues' conditions (T % 4 != 0,
    T < 128, segments of fewer than 256 rows; op level, bit for bit: tests/test_gpu_encoder_ops.py). d = 128 test model, 2 windows, audio_ctx 375, 130 and 100: the
    cross-K/V of the first and the last decoder layer from the timed path (T) against the exact mode's (E0), held to the floor measured in the same run exactly as
    test_timed_path_against_the_exact_mode holds the logits: max and mean |T - E0| within 1.5 x of |E0alt - E0|, E0alt being E0 with the weight products' 32 chains
    added left to right (option exact_alt_order), the smallest re-ordering of the reference's own FP32 sums. Then back to audio_ctx 0: the full-size caches are
    the bits they were before."""
    import bench
    model = gf.synth_model("test-d128", seed=1234, attn_sharpness=2.0)
    hp = model.hparams
    m = binding.HipModel.from_ggml(model)
    ctx = binding.HipContext(m, 2)
    pcm_dev = torch.from_numpy(bench.synth_pcm(2, seed=100)).cuda()
    mels = torch.stack([ctx.mel_spectrogram(pcm_dev[b]) for b in range(2)])
    layers = (0, hp.n_text_layer - 1)
    X = binding.WH_FLAG_PARITY_EXACT

    def caches(flags, n_ctx):
        ctx.set_flags(*flags)
        ctx.encode(mels)
        n = 2 * n_ctx * hp.n_audio_state         # [windows][audio_ctx][d], packed at the front of the full-size host array
        got = np.stack([np.asarray(ctx.debug_read(what, layer), np.float32).reshape(-1)[:n] for layer in layers for what in ("cross-k", "cross-v")])
        ctx.set_flags(0, 1)
        return got

    def dist(a, b):
        d = np.abs(a - b)
        return float(d.max()), float(d.mean())

    full = caches((0, 1), hp.n_audio_ctx)
    try:
        for n_ctx in (375, 130, 100):
            ctx.set_audio_ctx(n_ctx)
            T = caches((0, 1), n_ctx)
            E0 = caches((X, 0), n_ctx)
            binding.set_option("exact_alt_order", 1)
            try:
                E0alt = caches((X, 0), n_ctx)
            finally:
                binding.set_option("exact_alt_order", 0)
            floor_max, floor_mean = dist(E0alt, E0)
            t_max, t_mean = dist(T, E0)
            print("audio_ctx %d, cross-K/V of decoder layers %d and %d: re-ordered reference vs E0 %.3e / %.3e; timed vs E0 %.3e / %.3e (max / mean)"
                  % (n_ctx, layers[0], layers[1], floor_max, floor_mean, t_max, t_mean))
            assert np.isfinite(T).all() and np.isfinite(E0).all()
            assert t_max <= 1.5 * floor_max and t_mean <= 1.5 * floor_mean, (n_ctx, t_max, t_mean, floor_max, floor_mean)
        ctx.set_audio_ctx(0)
        again = caches((0, 1), hp.n_audio_ctx)
        assert np.array_equal(again, full), "the full-size caches changed after a round trip through reduced audio contexts"
    finally:
        ctx.close()
        m.close()


def test_exact_decoder_scratch_is_freed_when_it_grows():
    """The exact decoder's score scratch holds seqs * H * N * max(audio_ctx, n_past + N) floats, so with a small audio_ctx it grows while a host-stepped
    decode advances. A buffer that is replaced is given back: with U = 4 * seqs * n_text_head bytes, the two-token prompt at n_past = 0 needs 4 U, the steps
    at n_past = 4 .. 9 need 5 .. 10 U. Keeping every replaced buffer adds (5 + .. + 10) U = 4.5 S after the first step, S = 10 U being the final need; freeing on
    growth adds at most (16 - 4) U = 1.2 S with doubling. The bound is 2 S. The row buffers are sized by the prompt step and do not grow afterwards.
    Reallocation must not lose state: the last logits equal those of a context that decodes the same tokens after a step large enough to size every buffer
    once, so that nothing is reallocated under it."""
    model = gf.synth_model("test-d128", seed=1234, attn_sharpness=2.0)
    hp = model.hparams
    sp = gf.special_tokens(hp)
    import bench
    seqs = 2
    m = binding.HipModel.from_ggml(model)
    pcm_dev = torch.from_numpy(bench.synth_pcm(seqs, seed=100)).cuda()
    prompt = np.array([_prompt(sp)[:2]] * seqs, np.int32)
    steps = [np.full((seqs, 1), 1000 + 7 * k, np.int32) for k in range(8)]      # fed at n_past = 2 .. 9

    def start(presize):
        ctx = binding.HipContext(m, seqs)
        mels = torch.stack([ctx.mel_spectrogram(pcm_dev[b]) for b in range(seqs)])
        ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)
        ctx.set_audio_ctx(1)
        ctx.encode(mels)
        if presize:
            ctx.decode(np.zeros((seqs, 10), np.int32), 0)      # 10 x 10 scores per head, 20 rows: more than any call below; positions 0 .. 9 are rewritten
        return ctx

    ctx = start(False)
    ctx.decode(prompt, 0)
    v1 = ctx.vram_bytes()
    for k, t in enumerate(steps):
        logits, probs = ctx.decode(t, 2 + k)
    v = ctx.vram_bytes()
    S = 4 * seqs * hp.n_text_head * 10
    print("exact decoder scratch: vram grew by %d bytes over the steps at n_past = 2 .. 9; S = %d, bound 2 S = %d" % (v - v1, S, 2 * S))
    assert v - v1 <= 2 * S
    ctx.close()

    ref_ctx = start(True)
    v0 = ref_ctx.vram_bytes()
    ref_ctx.decode(prompt, 0)
    for k, t in enumerate(steps):
        ref_logits, ref_probs = ref_ctx.decode(t, 2 + k)
    assert ref_ctx.vram_bytes() == v0, "the comparison context was meant not to reallocate"
    assert np.isfinite(logits).all()
    assert np.array_equal(logits, ref_logits) and np.array_equal(probs, ref_probs)
    ref_ctx.close()
    m.close()
