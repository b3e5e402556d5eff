"""GPU tests, op level, of the kernels only a single-token decode step launches: gemvSmall, crossScores / crossSoftmaxPV (decode1.hip: 1 .. 4 sequences) and
selfBlockDec (attn_dec.hip: 9 .. 32 sequences), each against the float64 restatement of tests/decode_step_ref.py (pinned on the CPU by test_decode_step_ref_cpu.py).

Every call goes through the C ABI (wh_op_gemv_small, wh_op_cross_split, wh_op_self_block_dec). Outputs start as NaN, cache rows at or beyond the live key count are NaN,
and whatever a kernel must not write is compared bit for bit with what it held before the call. Every printed line carries the measured distance next to its bound.
"""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import decode_step_ref as ds  # noqa: E402
from oracle import whisper_np as wn  # noqa: E402
from whisper_amd import binding  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN32 = np.array([np.nan], F32).view(np.uint32)[0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def nan_f32(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def nan_f16(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float16, device="cuda")


def bits16(t):
    return t.cpu().numpy().view(np.uint16)


def ulp16(a):
    """One FP16 ulp at |a|, never less than the ulp of the smallest normal number."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(a), 2.0 ** -14))) - 10)


# ---- teacher forcing, as in test_gpu_ops.py: every stage of a fused kernel is held to the float64 restatement on the FP16 values the device itself produced one
# stage earlier, read back exactly through identity weights or unit-vector keys (1 . x + 0 + .. is exact). An FP32 LayerNorm lands a few activations per
# thousand on the other side of an FP16 rounding boundary than the float64 one does; such a row moves every product that reads it by ulp( x_k ) |w_k|, many ulps
# of a small output, and would be indistinguishable from a wrong sum downstream. ----
def check_layer_norm_rows(name, xn_dev, x, lnw, lnb):
    """test_layer_norm's criterion: FP16 values, each within one FP16 ulp of fp16( float64 LayerNorm ), fewer than 0.5 % different."""
    xn64 = ds.layer_norm16(x, lnw, lnb, np.float64)
    dx = np.abs(xn_dev - xn64)
    print("%s LayerNorm rows: %d of %d differ from fp16( float64 LayerNorm ), max %.2e (one FP16 ulp at most, fewer than 0.5 %%)" % (name, int((dx > 0).sum()), dx.size, dx.max()))
    assert np.array_equal(xn_dev, wn.r16(xn_dev)) and (dx <= ulp16(xn64)).all() and (dx > 0).mean() < 5e-3, name + ": LayerNorm rows"


def sum_roundoff(x16, w16, bias=None):
    """What FP32 accumulation in ANY order can move sum_k w[n][k] x[m][k] (+ bias) by: K 2^-24 ( sum |w x| + |bias| ), [M][N]."""
    t = np.abs(x16.astype(np.float64)) @ np.abs(w16.astype(np.float64)).T
    if bias is not None:
        t = t + np.abs(bias)
    return x16.shape[-1] * 2.0 ** -24 * t


def check_fp16_rows(name, got, want64, roundoff, literal=None):
    """got = fp16( want64 + e ), |e| <= roundoff: within one FP16 ulp of fp16( want64 ) plus the round-off of the sum (which only matters for elements so small
    that their ulp is below it: fewer than 1 % may be more than one ulp away). literal: the restatement from the float64 LayerNorm, printed for comparison."""
    want = wn.r16(want64)
    dd = np.abs(got - want)
    far = dd > ulp16(want)
    msg = "%s: %d of %d differ, %d by more than one FP16 ulp, max %.2e (bound: one ulp + FP32 round-off of the sum, largest %.2e)" % (name, int((dd > 0).sum()), dd.size, int(far.sum()), dd.max(), roundoff.max())
    if literal is not None:
        dl = np.abs(got - literal)
        msg += "; from the float64 LayerNorm instead: %d differ, %d by more than one ulp, max %.2e" % (int((dl > 0).sum()), int((dl > ulp16(literal)).sum()), dl.max())
    print(msg)
    assert np.array_equal(got, wn.r16(got)) and (dd <= ulp16(want) + roundoff).all() and far.mean() < 0.01, name


def gemv_small(M, N, K, epi, pro, w, a=None, ln=None, part=None, bias=None, res=None, out32=None, out16=None, q=None, kc=None, vc=None, heads=0, text_ctx=0,
               n_past=0, n_past_dev=None, scale=1.0):
    lnx, lnw, lnb = ln if ln is not None else (None, None, None)
    binding.check(binding.lib().wh_op_gemv_small(None, M, N, K, epi, pro, ptr(w), ptr(a), ptr(lnx), ptr(lnw), ptr(lnb), ptr(part), ptr(bias), ptr(res), ptr(out32),
                                                 ptr(out16), ptr(q), ptr(kc), ptr(vc), heads, text_ctx, n_past, ptr(n_past_dev), C.c_float(float(scale))))


# ----------------------------------------------------------------------------------------------------------------------
# gemvSmall, FP32 epilogue
# ----------------------------------------------------------------------------------------------------------------------
# K below one 1 KiB piece (384), ending inside a piece (768, 1280), the 16 pieces a lane can hold (8192), a ragged N (130, 51865, 51866), one row (N = 1)
GEMV_PAIRS = [(384, 384), (130, 512), (768, 768), (3840, 1280), (1024, 4096), (1280, 5120), (64, 8192), (1, 1024), (51865, 1024), (51866, 1280)]
# every pair at one and at three rows (the four-row instance with a missing row); two and four rows at three or more pairs each
GEMV_CASES = [(m, n, k) for (n, k) in GEMV_PAIRS for m in (1, 3)] + \
             [(2, 384, 384), (2, 3840, 1280), (2, 64, 8192), (2, 1, 1024), (4, 130, 512), (4, 768, 768), (4, 1024, 4096), (4, 51865, 1024)]


@functools.lru_cache(maxsize=2)
def _gemv_weights(N, K):
    """test_mul_mat's scales: weights 0.05 N(0,1), bias N(0,1). One matrix per (N, K), shared by the cases of that pair (the list is grouped by pair)."""
    rng = np.random.default_rng(N * 7 + K)
    w = (0.05 * rng.standard_normal((N, K), dtype=F32)).astype(np.float16)
    bias = rng.standard_normal(N).astype(F32)
    return w, bias, dev(w), dev(bias)


def _synthetic_partials(rng, M, H):
    """[M][H][8][68]: per (row, head) eight 64-vectors with their double sums; one split of each is the empty key range (sum 0, zero vector)."""
    part = np.zeros((M, H, ds.CROSS_SPLITS, ds.CROSS_PART), F32)
    sums = rng.uniform(0.2, 3.0, (M, H, ds.CROSS_SPLITS))
    vec = rng.standard_normal((M, H, ds.CROSS_SPLITS, 64)) * sums[..., None] * 2.6
    empty = (np.arange(M)[:, None] + np.arange(H)[None, :]) % ds.CROSS_SPLITS
    mi, hi = np.meshgrid(np.arange(M), np.arange(H), indexing="ij")
    sums[mi, hi, empty] = 0.0
    vec[mi, hi, empty] = 0.0
    part[..., :64] = vec
    part[..., 64:66] = np.ascontiguousarray(sums)[..., None].view(F32)
    part[..., 66:] = np.nan                       # the two padding floats are never read
    return part


@pytest.mark.parametrize("M,N,K", sorted(GEMV_CASES, key=lambda c: (c[1], c[2], c[0])))
def test_gemv_small_f32(M, N, K):
    """out = W x + bias + residual with FP32 accumulation, for the three ways gemvSmall builds x, against the float64 product of the same FP16 operands:
    test_mul_mat's bound at its input scales, 2e-5 max(1, sqrt(K / 128)). Rows beyond M are never written; repeated launches give the same bits."""
    w, bias, wd, bd = _gemv_weights(N, K)
    rng = np.random.default_rng(M * 131 + N + K)
    bound = 2e-5 * max(1.0, np.sqrt(K / 128))
    res = rng.standard_normal((M, N)).astype(F32)
    rd = dev(res)
    w64 = w.astype(np.float64)

    def run(pro, **kw):
        outs = []
        for rep in range(2):
            out = nan_f32(M + 1, N)
            gemv_small(M, N, K, 0, pro, wd, bias=bd, res=rd, out32=out, **kw)
            outs.append(out)
        torch.cuda.synchronize()
        got = outs[0].cpu().numpy()
        assert torch.equal(outs[0][:M], outs[1][:M]), "two launches differ"
        assert np.isnan(got[M]).all(), "a row beyond M was written"
        return got[:M]

    def held(name, got, x16):
        want = x16.astype(np.float64) @ w64.T + bias + res
        d = np.abs(got - want).max()
        print("gemv_small %dx%dx%d %-22s max|diff| %.3e (bound %.3e)" % (M, N, K, name, d, bound))
        assert np.isfinite(got).all() and d <= bound
        return want

    # ---- pro 0: FP16 activation rows ----
    a = rng.standard_normal((M, K)).astype(np.float16)
    ad = dev(a)
    got0 = run(0, a=ad)
    held("FP16 rows", got0, a.astype(F32))
    mm = nan_f32(M, N)
    binding.check(binding.lib().wh_op_mul_mat(None, ptr(ad), ptr(wd), ptr(bd), ptr(rd), ptr(mm), M, N, K))
    torch.cuda.synchronize()
    print("gemv_small %dx%dx%d against wh_op_mul_mat on the same operands: max|diff| %.3e" % (M, N, K, np.abs(got0 - mm.cpu().numpy()).max()))

    # ---- pro 1: LayerNorm prologue. The FP16 rows the kernel builds are read back through an identity weight (1 . x + 0 is exact), held to the float64
    # LayerNorm by test_layer_norm's criterion, and then used as the operands of the float64 product ----
    if K <= 2048:
        x = (rng.standard_normal((M, K)) * 2 + 0.3).astype(F32)
        lnw = (1 + 0.1 * rng.standard_normal(K)).astype(F32)
        lnb = (0.1 * rng.standard_normal(K)).astype(F32)
        ln = (dev(x), dev(lnw), dev(lnb))
        eye = dev(np.eye(K, dtype=np.float16))
        probe = nan_f32(M, K)
        gemv_small(M, K, K, 0, 1, eye, ln=ln, out32=probe)
        torch.cuda.synchronize()
        xn_dev = probe.cpu().numpy()
        check_layer_norm_rows("gemv_small %dx%dx%d" % (M, N, K), xn_dev, x, lnw, lnb)
        got1 = run(1, ln=ln)
        # a row whose activations all equal fp16( float64 LayerNorm ) -- 43 of the 46 rows of these cases -- is thereby held to the product of exactly that reference;
        # one activation that rounds the other way moves the row's outputs by ulp( x_k ) |w[n][k]|, up to 2e-4 at these scales (4 x 51865 x 1024: 1.98e-4)
        xn64 = ds.layer_norm16(x, lnw, lnb, np.float64)
        d64 = np.abs(got1 - (xn64.astype(np.float64) @ w64.T + bias + res)).max(axis=1)
        print("gemv_small %dx%dx%d LayerNorm prologue, operands = fp16( float64 LayerNorm ): max|diff| %.3e; rows with an activation on the other side of an FP16 boundary: %s"
              % (M, N, K, d64.max(), [int(r) for r in np.nonzero((xn_dev != xn64).any(axis=1))[0]]))
        held("LayerNorm prologue", got1, xn_dev)

    # ---- pro 3: the cross-attention partials combined in the kernel's stated order (ds.combine_partials at float32 is that arithmetic) ----
    part = _synthetic_partials(rng, M, K // 64)
    got3 = run(3, part=dev(part))
    held("partials combined", got3, ds.combine_partials(part, np.float32))


# ----------------------------------------------------------------------------------------------------------------------
# gemvSmall, GELU epilogue
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,d", [(1, 384), (2, 384), (3, 384), (4, 384), (1, 1280), (2, 1280), (3, 1280), (4, 1280)])
def test_gemv_small_gelu(M, d, golden):
    """The MLP up-projection of a single-token step: fp16 table GELU of ( acc + bias ), test_mul_mat_gelu's inputs and criterion."""
    N, K = 4 * d, d
    rng = np.random.default_rng(5 + M + d)
    a = rng.standard_normal((M, K)).astype(np.float16)
    w = (0.2 * rng.standard_normal((N, K))).astype(np.float16)
    bias = rng.standard_normal(N).astype(F32)
    pre = a.astype(np.float64) @ w.astype(np.float64).T + bias
    want = ds.gelu_table(pre, golden["table_gelu"])
    out = nan_f16(M + 1, N)
    gemv_small(M, N, K, 1, 0, dev(w), a=dev(a), bias=dev(bias), out16=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(F32)
    assert np.isnan(got[M]).all() and np.isfinite(got[:M]).all()
    dd = np.abs(got[:M] - want)
    print("gemv_small gelu %dx%dx%d: %.4f of the entries differ (bound 0.02), max %.2e (one FP16 ulp)" % (M, N, K, (dd > 0).mean(), dd.max()))
    assert (dd > 0).mean() < 0.02 and (dd <= np.maximum(4e-3, np.abs(want) * 2.0 ** -10)).all()


# ----------------------------------------------------------------------------------------------------------------------
# gemvSmall, Q/K/V epilogue of the decoder
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,d", [(1, 384), (4, 384), (1, 1024), (4, 1024)])
def test_gemv_small_qkv_decode(M, d):
    """LayerNorm + the fused [3d][d] product + the cache append: q and the two appended rows within one FP16 ulp of the restatement, every other element of
    both caches with the bits it had before the call (the padding rows are NaN: compared as uint16)."""
    H, ctx_rows = d // 64, 448
    rng = np.random.default_rng(M + d)
    x = (rng.standard_normal((M, d)) * 2 + 0.3).astype(F32)
    lnw = (1 + 0.1 * rng.standard_normal(d)).astype(F32)
    lnb = (0.1 * rng.standard_normal(d)).astype(F32)
    wqkv = (rng.standard_normal((3 * d, d)) / np.sqrt(d)).astype(np.float16)
    bqkv = (0.1 * rng.standard_normal(3 * d)).astype(F32)
    bqkv[d:2 * d] = 0.0
    scale = F32(64.0 ** -0.25)
    q_w, k_w, v_w = ds.qkv(ds.layer_norm16(x, lnw, lnb), wqkv, bqkv, scale)
    ln = (dev(x), dev(lnw), dev(lnb))
    wd, bd = dev(wqkv), dev(bqkv)
    per_seq = [0, 5, 64, 447][:M] if M > 1 else [64]
    for name, pos in [("nPast %d" % p, [p] * M) for p in (0, 63, 447)] + [("per-sequence positions", per_seq)]:
        kc = (0.8 * rng.standard_normal((M, H, ctx_rows, 64))).astype(np.float16)
        vc = rng.standard_normal((M, H, ctx_rows, 64)).astype(np.float16)
        for s in range(M):
            kc[s, :, pos[s]:] = np.nan
            vc[s, :, pos[s]:] = np.nan
        kd, vd, qd = dev(kc), dev(vc), nan_f16(M + 1, d)
        scalar = not name.startswith("per")
        gemv_small(M, 3 * d, d, 2, 1, wd, ln=ln, bias=bd, q=qd, kc=kd, vc=vd, heads=H, text_ctx=ctx_rows, n_past=pos[0] if scalar else 0,
                   n_past_dev=None if scalar else dev(np.asarray(pos, np.int32)), scale=scale)
        torch.cuda.synchronize()
        qg = qd.cpu().numpy().astype(F32)
        kg, vg = kd.cpu().numpy(), vd.cpu().numpy()
        assert np.isnan(qg[M]).all()
        worst = [0.0]
        assert (np.abs(qg[:M] - q_w) <= ulp16(q_w)).all(), "q"
        for s in range(M):
            k_row, v_row = kg[s, :, pos[s]].reshape(d).astype(F32), vg[s, :, pos[s]].reshape(d).astype(F32)
            assert (np.abs(k_row - k_w[s]) <= ulp16(k_w[s])).all() and (np.abs(v_row - v_w[s]) <= ulp16(v_w[s])).all(), "appended rows of sequence %d" % s
            worst.append(max(np.abs(k_row - k_w[s]).max(), np.abs(v_row - v_w[s]).max()))
            kc[s, :, pos[s]] = kg[s, :, pos[s]]
            vc[s, :, pos[s]] = vg[s, :, pos[s]]
        assert np.array_equal(kg.view(np.uint16), kc.view(np.uint16)) and np.array_equal(vg.view(np.uint16), vc.view(np.uint16)), "a cache element outside the appended rows changed"
        print("gemv_small qkv d=%d M=%d %s: q, k, v rows within one FP16 ulp (largest |diff| of a k / v row %.2e), %d other cache elements unchanged"
              % (d, M, name, max(worst), kc.size * 2 - 2 * M * d))


# ----------------------------------------------------------------------------------------------------------------------
# FP16-subnormal weights
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 4])
def test_subnormal_weights_survive_the_products(M):
    """Weights in the FP16 subnormal range (multiples of 2^-24 below 6.1e-5: what dequantized Q4 / Q5 blocks with a small scale hold) against activations of
    64 N(0,1): the float64 result is ~0.05. FP32 accumulation is ~1e-6 relative, an instruction that flushed FP16 subnormal operands would return 0
    (relative 1.0); the bound 1e-3 max|want| only has to separate the two -- for gemvSmall (v_dot2_f32_f16) and for the batch kernel (MFMA) on the same operands."""
    N, K = 256, 1024
    rng = np.random.default_rng(40 + M)
    w = (rng.integers(-1023, 1024, (N, K)).astype(np.float64) * 2.0 ** -24).astype(np.float16)
    assert (np.abs(w.astype(F32)) < 6.1e-5).all() and (w != 0).mean() > 0.99
    a = (64.0 * rng.standard_normal((M, K))).astype(np.float16)
    want = a.astype(np.float64) @ w.astype(np.float64).T
    ad, wd = dev(a), dev(w)
    got = {}
    out = nan_f32(M, N)
    gemv_small(M, N, K, 0, 0, wd, a=ad, out32=out)
    torch.cuda.synchronize()
    got["wh_op_gemv_small"] = out.cpu().numpy()
    out = nan_f32(M, N)
    binding.check(binding.lib().wh_op_mul_mat(None, ptr(ad), ptr(wd), None, None, ptr(out), M, N, K))
    torch.cuda.synchronize()
    got["wh_op_mul_mat"] = out.cpu().numpy()
    bound = 1e-3 * np.abs(want).max()
    dist = {k: np.abs(v - want).max() for k, v in got.items()}
    for k, v in dist.items():
        print("subnormal weights, M=%d, %s: max|want| %.4f, max|diff| %.3e = %.2e relative (bound %.3e)" % (M, k, np.abs(want).max(), v, v / np.abs(want).max(), bound))
    assert dist["wh_op_mul_mat"] <= bound
    assert dist["wh_op_gemv_small"] <= bound


# ----------------------------------------------------------------------------------------------------------------------
# cross-attention over eight key ranges
# ----------------------------------------------------------------------------------------------------------------------
def _cross_inputs(seqs, heads, n_keys, stride, seed):
    rng = np.random.default_rng(seed)
    d = heads * 64
    x = (rng.standard_normal((seqs, d)) * 2 + 0.3).astype(F32)
    lnw = (1 + 0.1 * rng.standard_normal(d)).astype(F32)
    lnb = (0.1 * rng.standard_normal(d)).astype(F32)
    wq = (rng.standard_normal((d, d), dtype=F32) / np.sqrt(d)).astype(np.float16)
    bq = (0.1 * rng.standard_normal(d)).astype(F32)
    K = (0.8 * rng.standard_normal((seqs, heads, stride, 64), dtype=F32)).astype(np.float16)
    V = rng.standard_normal((seqs, heads, stride, 64), dtype=F32).astype(np.float16)
    K[:, :, n_keys:] = np.nan
    V[:, :, n_keys:] = np.nan
    return x, lnw, lnb, wq, bq, F32(64.0 ** -0.25), K, V


def _run_cross_split(x, lnw, lnb, wq, bq, scale, K, V, n_keys, stride):
    """Both launches on NaN-filled scratch with one guard block behind each buffer. Returns scores [seqs][H][stride], splitMax [seqs][H][8], part [seqs][H][8][68]
    after checking that nothing outside the live region was written."""
    seqs, d = x.shape
    H = d // 64
    scores, smax, part = nan_f32(seqs + 1, H, stride), nan_f32(seqs + 1, H, 8), nan_f32(seqs + 1, H, 8, ds.CROSS_PART)
    ops = [dev(t) for t in (x, lnw, lnb, wq, bq)]
    kd, vd = dev(K), dev(V)
    binding.check(binding.lib().wh_op_cross_split(None, ptr(ops[0]), ptr(ops[1]), ptr(ops[2]), ptr(ops[3]), ptr(ops[4]), C.c_float(float(scale)), ptr(kd), ptr(vd),
                                                  ptr(scores), ptr(smax), ptr(part), seqs, H, n_keys, stride))
    torch.cuda.synchronize()
    sc, sm, pt = scores.cpu().numpy(), smax.cpu().numpy(), part.cpu().numpy()
    untouched = lambda a: (a.view(np.uint32) == NAN32).all()          # noqa: E731
    assert untouched(sc[seqs]) and untouched(sm[seqs]) and untouched(pt[seqs]), "a block behind the last sequence was written"
    assert untouched(sc[:seqs, :, n_keys:]), "scores beyond nKeys were written"
    assert untouched(pt[:seqs, :, :, 66:]), "the padding of a partial result was written"
    return sc[:seqs], sm[:seqs], pt[:seqs], ops, kd, vd


CROSS_KEYS = [1, 4, 5, 9, 28, 29, 32, 33, 700, 1499, 1500, 1536]
# every key count once at 20 heads x 3 sequences (strides alternate between the key count and 1536), the other widths and sequence counts sampled
CROSS_CASES = [(3, 20, n, n if i % 2 == 0 else 1536) for i, n in enumerate(CROSS_KEYS)] + \
              [(1, 6, 1, 1536), (1, 6, 29, 29), (1, 6, 1500, 1500), (4, 6, 33, 1536), (4, 6, 1536, 1536), (4, 16, 5, 5), (4, 16, 700, 1536), (4, 16, 1500, 1500),
               (1, 16, 28, 1536), (1, 20, 1499, 1499), (4, 20, 9, 1536)]


@pytest.mark.parametrize("seqs,heads,n_keys,stride", CROSS_CASES)
def test_cross_split(seqs, heads, n_keys, stride):
    """crossScores + crossSoftmaxPV against the float64 restatement. Key counts of 28 and fewer leave trailing ranges empty (maximum -inf, sum 0, zero vector).
    Stage by stage: the LayerNorm rows and the query are read back through keys that are unit vectors (K[j] = e_j gives score j = q[j] exactly; an identity query
    weight gives q = the LayerNorm row) and held to the restatement; the scores are held to the float64 products of the device's own query with the keys -- the
    FP32 round-off of a 64-term dot product, 64 * 2^-24 * sum |q_i k_i| -- so that an FP16 rounding of q that went the other way (worth 2e-4 in a score) is not
    mistaken for, and cannot hide, a wrong sum; the range maxima are exactly those of the device's scores; the combined output is held to the restatement
    computed from the inputs alone (float64 LayerNorm included) at the fused-query bounds, and to attentionDecG on the same inputs."""
    inp = _cross_inputs(seqs, heads, n_keys, stride, seqs * 1000 + heads * 10 + n_keys)
    x, lnw, lnb, wq, bq, scale, K, V = inp
    d = heads * 64
    # ---- the device's LayerNorm rows (identity query weight, no bias, scale 1: q = the row) and the device's query ----
    eyeK = np.zeros((seqs, heads, 64, 64), np.float16)
    eyeK[:, :] = np.eye(64, dtype=np.float16)
    xn_dev = _run_cross_split(x, lnw, lnb, np.eye(d, dtype=np.float16), np.zeros(d, F32), 1.0, eyeK, eyeK, 64, 64)[0].reshape(seqs, d)
    check_layer_norm_rows("cross_split s=%d h=%d keys=%d/%d" % (seqs, heads, n_keys, stride), xn_dev, x, lnw, lnb)
    q_dev = _run_cross_split(x, lnw, lnb, wq, bq, scale, eyeK, eyeK, 64, 64)[0].reshape(seqs, d)
    q_lit = ds.cross_query(x, lnw, lnb, wq, bq, scale)
    acc = xn_dev.astype(np.float64) @ wq.astype(np.float64).T
    check_fp16_rows("   query", q_dev, (acc + bq) * np.float64(scale), sum_roundoff(xn_dev, wq, bq) * float(scale), q_lit)
    # ---- scores, range maxima ----
    sc, sm, pt, ops, kd, vd = _run_cross_split(*inp, n_keys, stride)
    assert np.isfinite(sc[:, :, :n_keys]).all() and np.isfinite(pt[..., :66]).all()
    k64 = K[:, :, :n_keys].astype(np.float64)
    qh = q_dev.reshape(seqs, heads, 64).astype(np.float64)
    want_sc = np.einsum("shkj,shj->shk", k64, qh)
    sc_bound = 64 * 2.0 ** -24 * np.einsum("shkj,shj->shk", np.abs(k64), np.abs(qh))
    ds_ = np.abs(sc[:, :, :n_keys] - want_sc)
    print("   scores: max|diff| %.3e (bound per score, largest %.3e; worst ratio %.3f)" % (ds_.max(), sc_bound.max(), (ds_ / np.maximum(sc_bound, 1e-30)).max()))
    assert (ds_ <= sc_bound).all()
    ranges = ds.split_ranges(n_keys)
    for i, (a, b) in enumerate(ranges):
        want_max = sc[:, :, a:b].max(axis=2) if b > a else np.full((seqs, heads), -np.inf, F32)
        assert np.array_equal(sm[:, :, i], want_max), "maximum of range %d" % i
        if b == a:
            assert not pt[:, :, i, :66].any(), "an empty range left a sum"
    # ---- the attention output: the partials combined on the host in the kernel's order ----
    got = ds.combine_partials(pt, np.float32)
    _, want = ds.cross_split(x, lnw, lnb, wq, bq, scale, K, V, n_keys)
    dd = np.abs(got - want)
    ref_out = nan_f16(seqs, d)
    binding.check(binding.lib().wh_op_decoder_cross_attention(None, ptr(ops[0]), ptr(ops[1]), ptr(ops[2]), ptr(ops[3]), ptr(ops[4]), C.c_float(float(scale)), ptr(kd), ptr(vd),
                                                              ptr(ref_out), seqs, heads, n_keys, stride, 1))
    torch.cuda.synchronize()
    db = np.abs(got - ref_out.cpu().numpy().astype(F32))
    print("   output: max|diff| %.2e (bound 4e-3) mean %.2e (bound 3e-4); against wh_op_decoder_cross_attention max %.2e (bound 4e-3)" % (dd.max(), dd.mean(), db.max()))
    assert np.isfinite(got).all() and dd.max() < 4e-3 and dd.mean() < 3e-4
    assert db.max() < 4e-3
    # ... and through the consumer itself: gemvSmall's combine prologue against an identity weight returns the same FP16 rows
    if n_keys in (28, 1500):
        out = nan_f32(seqs, d)
        gemv_small(seqs, d, d, 0, 3, dev(np.eye(d, dtype=np.float16)), part=dev(pt), out32=out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), got), "gemvSmall's combine differs from the stated order"


@pytest.mark.parametrize("n_keys,stride", [(1500, 1500), (9, 1536), (29, 29)])
def test_cross_split_maximum_alone_in_the_last_range(n_keys, stride):
    """The last key of the last non-empty range scores 25 above every other key, which all score within +-1 of 0: every other exponential is
    fp16( exp( -24 ) ) = 0, seven ranges sum to 0 and contribute zero vectors, and the output is that key's value row, exactly."""
    seqs, heads = 3, 20
    x, lnw, lnb, wq, bq, scale, K, V = _cross_inputs(seqs, heads, n_keys, stride, 77 + n_keys)
    q = ds.cross_query(x, lnw, lnb, wq, bq, scale).reshape(seqs, heads, 64)
    K[:, :, :n_keys] = (K[:, :, :n_keys].astype(F32) * 0.02).astype(np.float16)
    K[:, :, n_keys - 1] = (q * (25.0 / (q.astype(np.float64) ** 2).sum(axis=2, keepdims=True))).astype(np.float16)
    sc, sm, pt, _, _, _ = _run_cross_split(x, lnw, lnb, wq, bq, scale, K, V, n_keys, stride)
    top = sc[:, :, n_keys - 1]
    others = sc[:, :, :n_keys - 1]
    print("adversarial keys=%d: top score %.2f .. %.2f, every other |score| <= %.2f" % (n_keys, top.min(), top.max(), np.abs(others).max() if n_keys > 1 else 0.0))
    assert top.min() > 24.0 and np.abs(others).max() < 1.0
    last = max(i for i, (a, b) in enumerate(ds.split_ranges(n_keys)) if b > a)
    assert np.isfinite(pt[..., :66]).all()
    for i in range(8):
        if i != last:
            assert not pt[:, :, i, :66].any(), "range %d should sum to zero" % i
    got = ds.combine_partials(pt, np.float32)
    assert np.isfinite(got).all()
    assert np.array_equal(got, V[:, :, n_keys - 1].astype(F32).reshape(seqs, heads * 64))


# ----------------------------------------------------------------------------------------------------------------------
# selfBlockDec
# ----------------------------------------------------------------------------------------------------------------------
SELF_VARIANTS = [(1, True), (1, False), (2, True), (2, False), (4, True), (4, False), (8, True)]      # (self_nq, TUNE_SELF_MFMA); 8 per workgroup exists on the matrix cores only
MIXED = [0, 63, 64, 447, 447, 0, 64, 63, 1, 65, 128, 200, 447]                                       # 0, 63, 64 and 447 inside one group of 4 (and of 8); pairs (0, 63), (64, 447)
# 13 sequences: the last workgroup of 2, 4 and 8 per group is ragged. Every case runs every variant, so each variant sees positions 0, 64, 447 and a ragged group.
SELF_CASES = [(2, 13, 0), (2, 13, 64), (2, 13, 447), (2, 9, 1), (2, 1, 63), (2, 32, 65), (2, 9, 127), (2, 13, 128), (2, 32, 200), (2, 13, MIXED),
              (16, 13, MIXED), (16, 9, 64), (16, 1, 447), (16, 32, 0), (16, 13, 65),
              (20, 13, MIXED), (20, 32, 447), (20, 9, 63), (20, 1, 128), (20, 13, 0), (20, 13, 64), (20, 32, MIXED + MIXED + [127, 128, 0, 64, 447, 63])]


@pytest.mark.parametrize("heads,seqs,positions", SELF_CASES, ids=lambda v: "mixed" if isinstance(v, list) else str(v))
def test_self_block_dec(heads, seqs, positions):
    """LayerNorm -> Q/K/V rows of a head -> append -> causal attention in one launch, 1 / 2 / 4 / 8 sequences per workgroup, projection on the matrix cores or the
    VALU: the output within the fused-query bound of the restatement (4e-3 max, 3e-4 mean: the same extra rounding points), the LayerNorm rows (read back through
    identity weights) by test_layer_norm's criterion, the appended rows within one FP16 ulp of the restatement on those rows, every other cache element untouched,
    the variants within 4e-3 of each other. The score loop's 64-row passes end at 64 and 128, the deepest position is 447."""
    d, stride = heads * 64, 448
    scalar = not isinstance(positions, list)
    pos = [positions] * seqs if scalar else list(positions[:seqs])
    assert len(pos) == seqs
    rng = np.random.default_rng(heads * 100 + seqs + sum(pos))
    x = (rng.standard_normal((seqs, d)) * 2 + 0.3).astype(F32)
    lnw = (1 + 0.1 * rng.standard_normal(d)).astype(F32)
    lnb = (0.1 * rng.standard_normal(d)).astype(F32)
    wqkv = (rng.standard_normal((3 * d, d), dtype=F32) / np.sqrt(d)).astype(np.float16)
    bqkv = (0.1 * rng.standard_normal(3 * d)).astype(F32)
    bqkv[d:2 * d] = 0.0
    scale = F32(64.0 ** -0.25)
    kc = (0.8 * rng.standard_normal((seqs, heads, stride, 64), dtype=F32)).astype(np.float16)
    vc = rng.standard_normal((seqs, heads, stride, 64), dtype=F32).astype(np.float16)
    for s in range(seqs):
        kc[s, :, pos[s]:] = np.nan
        vc[s, :, pos[s]:] = np.nan
    want, k_lit, v_lit = ds.self_block(x, lnw, lnb, wqkv, bqkv, scale, kc, vc, pos)
    xd, lw, lb, wd, bd = dev(x), dev(lnw), dev(lnb), dev(wqkv), dev(bqkv)
    # the LayerNorm rows as the kernel builds them: with three identity blocks as the weight, no bias and scale 1 the appended K and V rows ARE the rows
    eye3, zero3 = dev(np.concatenate([np.eye(d, dtype=np.float16)] * 3)), dev(np.zeros(3 * d, F32))
    pos_dev = None if scalar else dev(np.asarray(pos, np.int32))
    L = binding.lib()

    def launch(weight, bias, s):
        kd, vd, out = dev(kc), dev(vc), nan_f16(seqs + 1, d)
        binding.check(L.wh_op_self_block_dec(None, ptr(xd), ptr(lw), ptr(lb), ptr(weight), ptr(bias), C.c_float(float(s)), ptr(kd), ptr(vd), ptr(out), seqs, heads, stride,
                                             pos[0] if scalar else 0, ptr(pos_dev)))
        torch.cuda.synchronize()
        return out.cpu().numpy().astype(F32), kd.cpu().numpy(), vd.cpu().numpy()

    def appended(cache):
        return np.stack([cache[s, :, pos[s]].reshape(d) for s in range(seqs)]).astype(F32)

    outs, rows = {}, {}
    try:
        for nq, mf in SELF_VARIANTS:
            L.wh_debug_set_tuning(binding.TUNE_DEFAULT | binding.TUNE_SELF_MFMA if mf else binding.TUNE_DEFAULT & ~binding.TUNE_SELF_MFMA)
            binding.set_option("self_nq", nq)
            _, kp, vp = launch(eye3, zero3, 1.0)
            rows[(nq, mf)] = (appended(kp), appended(vp))
            outs[(nq, mf)] = launch(wd, bd, scale)
    finally:
        L.wh_debug_set_tuning(binding.TUNE_DEFAULT)
        binding.set_option("self_nq", binding.get_option_default("self_nq"))
    w64 = wqkv.astype(np.float64)
    for (nq, mf), (got, kg, vg) in outs.items():
        name = "self_block_dec h=%d s=%d pos=%s nq=%d %s" % (heads, seqs, positions if scalar else "mixed", nq, "mfma" if mf else "valu")
        assert np.isnan(got[seqs]).all(), name + ": a row beyond the batch was written"
        got = got[:seqs]
        assert np.isfinite(got).all(), name
        xn_dev = rows[(nq, mf)][0]
        assert np.array_equal(xn_dev, rows[(nq, mf)][1]), name + ": the key and the value projection saw different LayerNorm rows"
        check_layer_norm_rows(name, xn_dev, x, lnw, lnb)
        # appended rows: k = fp16( W xn s ), v = fp16( W xn + b ) on the device's own rows
        acc = xn_dev.astype(np.float64) @ w64[d:].T
        check_fp16_rows("   appended K rows", appended(kg), acc[:, :d] * np.float64(scale), sum_roundoff(xn_dev, wqkv[d:2 * d]) * float(scale), k_lit)
        check_fp16_rows("   appended V rows", appended(vg), acc[:, d:] + bqkv[2 * d:], sum_roundoff(xn_dev, wqkv[2 * d:], bqkv[2 * d:]), v_lit)
        expect_k, expect_v = kc.copy(), vc.copy()
        for s in range(seqs):
            expect_k[s, :, pos[s]] = kg[s, :, pos[s]]
            expect_v[s, :, pos[s]] = vg[s, :, pos[s]]
        assert np.array_equal(kg.view(np.uint16), expect_k.view(np.uint16)) and np.array_equal(vg.view(np.uint16), expect_v.view(np.uint16)), name + ": a cache element outside the appended rows changed"
        # the output against the restatement from the inputs alone (float64 LayerNorm included)
        dd = np.abs(got - want)
        print("   output max %.2e (bound 4e-3) mean %.2e (bound 3e-4)" % (dd.max(), dd.mean()))
        assert dd.max() < 4e-3 and dd.mean() < 3e-4, name
    first = outs[SELF_VARIANTS[0]][0][:seqs]
    spread = max(np.abs(o[0][:seqs] - first).max() for o in outs.values())
    print("self_block_dec h=%d s=%d: the seven variants within %.2e of each other (bound 4e-3)" % (heads, seqs, spread))
    assert spread < 4e-3
