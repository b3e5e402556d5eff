"""The encoder's four fused products and the producer of conv1's operand, at op level, against exact references.

wh_encode builds conv1, conv2, Q/K/V and the cross-K/V of every decoder layer by hand (csrc/encode.hip): segmented and overlapping operand rows, outputs scattered
by head, by the attention's V operand order, by layer and window. wh_op_gemm_encoder hands the same arrangements to the same chooser (launchGemm) and says which
kernel family and which epilogue level took them; tests/encoder_ops_ref.py restates them in numpy. The inputs are dyadic (multiples of 1/8, 1/16, 1/128), so every
FP32 sum is exact in any order (tests/test_encoder_ops_ref_cpu.py) and what follows the sum is a fixed sequence of single roundings: the expected output is known
BIT FOR BIT, whatever the tile shape, the wave layout or the matrix instruction.

Every case: the outputs start as a sentinel (FP16 0x7BFF, FP32 NaN 0x7FC0BEEF) inside guard margins of the same; every live element must equal the reference, every
other element -- the guards, padded rows 0 and Mb + 1 of conv1's output, V's keys [T, Tpad), the cache windows before and after the chunk -- must still hold the
sentinel; the family and the epilogue level reported must be the ones the case was built to reach.

GELU: gelu16 is a pure function of the FP16 bits of its argument. Its 65536-entry map is the ONE scalar function these tests take from the device (read once through
the plain wh_op_mul_mat_gelu, the method of test_gpu_ops.py::test_gelu_table_exhaustive, which pins it to within one ulp of the reference's table on fewer than
0.2 % of the entries); at every argument a fused product actually hits, the map is additionally held to within one FP16 ulp of golden["table_gelu"] here.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import encoder_ops_ref as R  # noqa: E402
from whisper_amd import binding  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096                                                     # elements on either side of every output
B = binding
D = B.TUNE_DEFAULT
# name -> (tuning mask, gemm_mf16, the family a product of 300 tiles and 8192 rows must report); "t128" is for products below that
FAMILIES = {
    "t128": (D, 1, B.GEMM_TILED_128),
    "t128-narrow": (D & ~B.TUNE_GEMM_WIDE_EPI, 1, B.GEMM_TILED_128),
    "t256": (D & ~B.TUNE_GEMM_8WAVE, 1, B.GEMM_TILED_256),
    "t256-narrow": (D & ~B.TUNE_GEMM_8WAVE & ~B.TUNE_GEMM_WIDE_EPI, 1, B.GEMM_TILED_256),
    "t8-lean": (D, 1, B.GEMM_TILED8),
    "t8-lean-mf0": (D, 0, B.GEMM_TILED8),
    "t8-general": (D & ~B.TUNE_GEMM_FAST_EPI, 1, B.GEMM_TILED8),
    "t8-general-mf0": (D & ~B.TUNE_GEMM_FAST_EPI, 0, B.GEMM_TILED8),
    "t8-narrow": (D & ~B.TUNE_GEMM_WIDE_EPI, 1, B.GEMM_TILED8),
    "t4": (D | B.TUNE_GEMM_4WAVE, 1, B.GEMM_TILED4),
    "t4-narrow": ((D | B.TUNE_GEMM_4WAVE) & ~B.TUNE_GEMM_WIDE_EPI, 1, B.GEMM_TILED4),
}
FAMILY_NAMES = {B.GEMM_TILED_128: "gemmTiled 128", B.GEMM_TILED_256: "gemmTiled 256", B.GEMM_TILED8: "gemmTiled8", B.GEMM_TILED4: "gemmTiled4"}


@contextlib.contextmanager
def family(name):
    mask, mf16, _ = FAMILIES[name]
    L = B.lib()
    L.wh_debug_set_tuning(mask)
    B.set_option("gemm_mf16", mf16)
    B.set_option("gemm_big_min_rows", B.get_option_default("gemm_big_min_rows"))
    try:
        yield
    finally:
        L.wh_debug_set_tuning(B.TUNE_DEFAULT)
        B.set_option("gemm_mf16", B.get_option_default("gemm_mf16"))
        B.set_option("gemm_big_min_rows", B.get_option_default("gemm_big_min_rows"))


def expected_wide(fam, name, epi, T=0, H=0, Mb=0, segmented=False):
    """The epilogue level the launchers state for a family (gemm_tiled.hip launchTiledT, gemm_persistent.hip launchPersistent / fastEpilogueOk), every buffer here
    being 16-byte aligned: 0 = column stores, 1 = 16-byte row stores through LDS, 2 = that with the lean epilogue on interior tiles."""
    mask = FAMILIES[name][0]
    if not mask & B.TUNE_GEMM_WIDE_EPI:
        return 0
    if fam in (B.GEMM_TILED_128, B.GEMM_TILED_256):
        return 1
    heads = epi in (B.EPI_QKV_ENC, B.EPI_CROSS_KV)
    lean_ok = (T >= 128 and H % 2 == 0) if heads else (not segmented or Mb >= 128)
    if fam == B.GEMM_TILED4:
        if epi == B.EPI_QKV_ENC and T % 4:
            return 0                                            # its wide epilogue takes the V columns too: whole groups of 4 keys
        return 2 if lean_ok else 1
    lean = bool(mask & B.TUNE_GEMM_FAST_EPI) and (epi != B.EPI_QKV_ENC or T % 4 == 0)
    return 2 if lean and lean_ok else 1


class Out:
    """A device buffer of n 2- or 4-byte elements between two guard margins, everything pre-filled with the sentinel; read back as bit patterns."""

    def __init__(self, n, bits):
        self.n, self.np = int(n), (np.uint16 if bits == 16 else np.uint32)
        self.sentinel = R.SENTINEL16 if bits == 16 else R.SENTINEL32
        self.t = torch.full((self.n + 2 * GUARD,), int(self.sentinel), dtype=torch.int16 if bits == 16 else torch.int32, device="cuda")
        self.ptr = self.t.data_ptr() + GUARD * (bits // 8)
        assert self.ptr % 16 == 0

    def read(self, what):
        torch.cuda.synchronize()
        host = self.t.cpu().numpy().view(self.np)
        assert (host[:GUARD] == self.sentinel).all(), what + ": the guard below the buffer was written"
        assert (host[-GUARD:] == self.sentinel).all(), what + ": the guard above the buffer was written"
        return host[GUARD:-GUARD]


def same_bits(got, want, what):
    want = np.ascontiguousarray(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    if len(bad):
        i = int(bad[0])
        pytest.fail("%s: %d of %d elements differ, first at %d: got 0x%x want 0x%x (sentinel 0x%x)" %
                    (what, len(bad), len(want), i, int(got[i]), int(want[i]), int(R.SENTINEL16 if got.dtype == np.uint16 else R.SENTINEL32)))


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # a copy: the shared references are read-only


@pytest.fixture(scope="module")
def gelu_map():
    """gelu16 as the device computes it, over every finite FP16 argument (entries of the others: 0, never looked up)."""
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    fin = np.isfinite(x.view(np.float16))
    xs = x[fin].view(np.float16)
    a = np.zeros((len(xs), 64), np.float16)
    a[:, 0] = xs
    w = np.zeros((64, 64), np.float16)
    w[:, 0] = 1.0
    ad, wd, bd = dev(a), dev(w), dev(np.zeros(64, np.float32))
    out = torch.zeros((len(xs), 64), dtype=torch.float16, device="cuda")
    B.check(B.lib().wh_op_mul_mat_gelu(None, ad.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), len(xs), 64, 64))
    torch.cuda.synchronize()
    m = np.zeros(65536, np.uint16)
    m[fin] = out.cpu().numpy()[:, 3].view(np.uint16)
    return m


def gelu_within_one_ulp(arg_bits, gelu_map, golden, what):
    """The fused outputs equal gelu_map[ argument ] bit for bit (asserted by the caller), so holding the map to the reference's table at the arguments that occurred
    holds every fused output to it."""
    args = np.unique(arg_bits)
    assert np.isfinite(args.view(np.float16)).all()
    dist = R.f16_ulp_distance(gelu_map[args], golden["table_gelu"][args])
    print("%s: %d distinct GELU arguments, %d off the reference's table, at most %d ulp" % (what, len(args), int((dist > 0).sum()), int(dist.max())))
    assert dist.max() <= 1


# one reference per shape, shared by the families that follow it (the cases are ordered by shape); never modified
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE.clear()
        _CACHE[key] = make()
    return _CACHE[key]


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def report(what, name, fam, wide):
    print("%-44s %-15s -> %-13s wideEpi %d" % (what, name, FAMILY_NAMES[fam], wide))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Q/K/V
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def qkv_inputs(H, M, gaussian=False):
    d = 64 * H
    rng = np.random.default_rng(1000 + H * 7 + M)
    if gaussian:
        a, w = rng.standard_normal((M, d)).astype(np.float16), (0.05 * rng.standard_normal((3 * d, d))).astype(np.float16)
        bias = rng.standard_normal(3 * d).astype(np.float32)
        return frozen(a, w, bias, R.mul_acc(a, w))
    a, w, bias = R.activations(rng, (M, d)), R.weights(rng, (3 * d, d)), R.biases(rng, 3 * d)
    return frozen(a, w, bias, R.as_f32_exact(R.mul_acc(a, w)))


def run_qkv(a, w, bias, H, T, name):
    M, d = a.shape
    batch, Tpad = M // T, R.round_up(T, 256)
    ad, wd, bd = dev(a), dev(w), dev(bias)
    q, k, v = Out(M * d, 16), Out(M * d, 16), Out(batch * H * 64 * Tpad, 16)
    with family(name):
        fam, wide = B.op_gemm_encoder(a=ad.data_ptr(), w=wd.data_ptr(), bias=bd.data_ptr(), q=q.ptr, k=k.ptr, v=v.ptr, M=M, N=3 * d, K=d, lda=d, Mb=M, ldc=3 * d,
                                      epi=B.EPI_QKV_ENC, T=T, Tpad=Tpad, H=H, B=batch, scale=1.0)
    what = "Q/K/V d=%d %d x T=%d" % (d, batch, T)
    report(what, name, fam, wide)
    return fam, wide, q.read(what + " q"), k.read(what + " k"), v.read(what + " v"), what


QKV_BIG = ["t256", "t8-lean", "t8-lean-mf0", "t8-general"]
QKV_CASES = ([(2, 39000, T, n) for T in (1500, 375, 130, 100) for n in QKV_BIG + (["t256-narrow", "t8-narrow", "t8-general-mf0"] if T == 1500 else [])] +
             [(3, 25500, 1500, n) for n in QKV_BIG] +
             # K = 256: the smallest at which gemmTiled4 takes a product; T % 4 == 3 turns its wide epilogue (V included) off
             [(4, 25500, 1500, "t4"), (4, 25500, 1500, "t4-narrow"), (4, 25500, 375, "t4")] +
             [(2, 2 * T, T, n) for T in (1500, 375, 130, 100, 1) for n in ["t128"] + (["t128-narrow"] if T in (1500, 375) else [])] +
             [(3, 2 * 130, 130, "t128")])


@pytest.mark.parametrize("H,M,T,name", QKV_CASES)
def test_qkv(H, M, T, name):
    """EPI_QKV_ENC: head-split Q and K, V scattered through vFragIndex into [b][h][64 x Tpad]; V's keys [T, Tpad) keep the sentinel."""
    a, w, bias, acc = cached(("qkv", H, M), lambda: qkv_inputs(H, M))
    batch = M // T
    fam, wide, q, k, v, what = run_qkv(a, w, bias, H, T, name)
    wq, wk, wv = R.epi_qkv(acc.reshape(batch, T, -1), bias, H, R.round_up(T, 256))
    same_bits(q, wq, what + " q")
    same_bits(k, wk, what + " k")
    same_bits(v, wv, what + " v (keys beyond T untouched)")
    assert fam == (FAMILIES[name][2] if M >= 8192 else B.GEMM_TILED_128), (what, name, fam)
    assert wide == expected_wide(fam, name, B.EPI_QKV_ENC, T=T, H=H), (what, name, wide)


@pytest.mark.parametrize("M,name", [(39000, "t8-lean"), (39000, "t256"), (3000, "t128")])
def test_qkv_outputs_off_16_bytes_take_the_narrow_epilogue(M, name):
    """wideEpilogueOk: the 16-byte row stores need q and k on 16-byte boundaries. Eight bytes off, every family must say 0 and still put every element in its place."""
    H, T = 2, 1500
    a, w, bias, acc = cached(("qkv", H, M), lambda: qkv_inputs(H, M))
    d, batch, Tpad = 64 * H, M // T, R.round_up(T, 256)
    ad, wd, bd = dev(a), dev(w), dev(bias)
    q, k, v = Out(M * d + 8, 16), Out(M * d + 8, 16), Out(batch * H * 64 * Tpad, 16)
    with family(name):
        fam, wide = B.op_gemm_encoder(a=ad.data_ptr(), w=wd.data_ptr(), bias=bd.data_ptr(), q=q.ptr + 8, k=k.ptr + 8, v=v.ptr, M=M, N=3 * d, K=d, lda=d, Mb=M, ldc=3 * d,
                                      epi=B.EPI_QKV_ENC, T=T, Tpad=Tpad, H=H, B=batch, scale=1.0)
    what = "Q/K/V d=%d %d x T=%d, q and k 8 bytes off" % (d, batch, T)
    report(what, name, fam, wide)
    wq, wk, wv = R.epi_qkv(acc.reshape(batch, T, -1), bias, H, Tpad)
    pad = np.full(4, R.SENTINEL16, np.uint16)
    same_bits(q.read(what + " q"), np.concatenate([pad, wq.reshape(-1), pad]), what + " q")
    same_bits(k.read(what + " k"), np.concatenate([pad, wk.reshape(-1), pad]), what + " k")
    same_bits(v.read(what + " v"), wv, what + " v")
    assert fam == (FAMILIES[name][2] if M >= 8192 else B.GEMM_TILED_128) and wide == 0, (what, name, fam, wide)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# cross-K/V of every decoder layer
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def cross_inputs(H, layers, M, gaussian=False):
    d = 64 * H
    rng = np.random.default_rng(2000 + H * 7 + M + layers)
    if gaussian:
        a, w = rng.standard_normal((M, d)).astype(np.float16), (0.05 * rng.standard_normal((layers * 2 * d, d))).astype(np.float16)
        bias = rng.standard_normal(layers * 2 * d).astype(np.float32)
        return frozen(a, w, bias, R.mul_acc(a, w))
    a, w, bias = R.activations(rng, (M, d)), R.weights(rng, (layers * 2 * d, d)), R.biases(rng, layers * 2 * d)
    return frozen(a, w, bias, R.as_f32_exact(R.mul_acc(a, w)))


def cross_scale(H):
    return float(np.float32(np.power(np.float64(np.float32(64 * H) / np.float32(H)), -0.25)))


def run_cross(a, w, bias, H, T, b0, cap, name):
    M, d = a.shape
    N = w.shape[0]
    layers = N // (2 * d)
    ad, wd, bd = dev(a), dev(w), dev(bias)
    k, v = Out(layers * cap * T * d, 16), Out(layers * cap * T * d, 16)
    off = 2 * b0 * T * d                                       # bytes: the chunk's first window inside layer 0, as encodeImpl offsets the base pointers
    with family(name):
        fam, wide = B.op_gemm_encoder(a=ad.data_ptr(), w=wd.data_ptr(), bias=bd.data_ptr(), k=k.ptr + off, v=v.ptr + off, M=M, N=N, K=d, lda=d, Mb=M, ldc=N,
                                      epi=B.EPI_CROSS_KV, T=T, H=H, B=cap, scale=cross_scale(H))
    what = "cross-K/V d=%d %d layers %d x T=%d at %d of %d" % (d, layers, M // T, T, b0, cap)
    report(what, name, fam, wide)
    return fam, wide, k.read(what + " k"), v.read(what + " v"), what


CROSS_BIG = ["t256", "t8-lean", "t8-lean-mf0", "t8-general"]
CROSS_CASES = ([(2, 4, 19500, T, n) for T in (1500, 375, 100) for n in CROSS_BIG + (["t256-narrow", "t8-narrow"] if T == 1500 else [])] +
               [(4, 2, 19500, 1500, "t4"), (4, 2, 19500, 1500, "t4-narrow"), (4, 2, 19500, 100, "t4")] +
               [(3, 2, 2 * 130, 130, "t128"), (3, 2, 2 * 130, 130, "t128-narrow"), (2, 4, 2, 1, "t128")])


@pytest.mark.parametrize("H,layers,M,T,name", CROSS_CASES)
def test_cross_kv(H, layers, M, T, name):
    """EPI_CROSS_KV: [layer][B][h][T][64] written at a chunk offset of 2 windows; B = 16 at T = 1500 (3 more than the chunk holds elsewhere): the windows before and
    after the chunk, in every layer, keep the sentinel. K = fp16( acc * scale ), V = fp16( acc + bias )."""
    a, w, bias, acc = cached(("cross", H, layers, M), lambda: cross_inputs(H, layers, M))
    batch, b0 = M // T, 2
    cap = 16 if batch == 13 else batch + 3
    fam, wide, k, v, what = run_cross(a, w, bias, H, T, b0, cap, name)
    # the entry point is given the caches from window b0 on, with B = cap: the window index inside a layer is b0 + b of the full caches
    wk, wv = R.epi_cross(acc.reshape(batch, T, -1), bias, np.float32(cross_scale(H)), H, cap, b0)
    same_bits(k, wk, what + " k")
    same_bits(v, wv, what + " v")
    assert fam == (FAMILIES[name][2] if M >= 8192 else B.GEMM_TILED_128), (what, name, fam)
    assert wide == expected_wide(fam, name, B.EPI_CROSS_KV, T=T, H=H), (what, name, wide)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# conv1: an implicit GEMM over overlapping rows, into a segmented buffer one row in
# ---------------------------------------------------------------------------------------------------------------------------------------------------
GAP = 64                                                         # halves between two windows of conv1's operand, and after the last one
BIG16 = np.float16(32768.0)


def conv1_inputs(n_mels, d, batch, T, gaussian=False):
    """The operand as wh_encode lays it out, windows GAP halves apart: rows 0 and 2 T + 1 of a window zero, rows 1 .. 2 T live, and 32768 in every gap. The last row of
    a window reads conv1Kpad - 3 n_mels halves past its logical end, into the gap, against the zero padding of the weight rows (csrc/model.hip): a kernel that let the
    padding reach the sum, or weights that were not zero there, would show at once. (Inside a window the same over-read lands on live data of the row after next.)"""
    mb, kpad = 2 * T, R.round_up(3 * n_mels, 64)
    rng = np.random.default_rng(3000 + n_mels + T)
    xpad = np.zeros((batch, mb + 2, n_mels), np.float16)
    if gaussian:
        xpad[:, 1:-1] = rng.standard_normal((batch, mb, n_mels)).astype(np.float16)
        w_file, bias = (0.05 * rng.standard_normal((d, n_mels, 3))).astype(np.float16), rng.standard_normal(d).astype(np.float32)
    else:
        xpad[:, 1:-1] = R.activations(rng, (batch, mb, n_mels))
        w_file, bias = R.weights(rng, (d, n_mels, 3)), R.biases(rng, d)
    stride = (mb + 2) * n_mels + GAP
    flat = np.full((batch, stride), BIG16, np.float16)
    flat[:, :(mb + 2) * n_mels] = xpad.reshape(batch, -1)
    w_rows = R.conv_weight_rows(w_file, kpad)
    assert kpad - 3 * n_mels <= GAP and (w_rows[:, 3 * n_mels:] == 0).all() and np.isfinite(flat).all()
    acc = R.conv_acc(xpad, w_rows, 1)
    return frozen(flat, w_rows, bias, acc if gaussian else R.as_f32_exact(acc))


def run_conv1(flat, w_rows, bias, n_mels, T, name):
    batch, stride = flat.shape
    d, kpad = w_rows.shape
    mb = 2 * T
    ad, wd, bd = dev(flat), dev(w_rows), dev(bias)
    out = Out(batch * (mb + 2) * d, 16)
    with family(name):
        fam, wide = B.op_gemm_encoder(a=ad.data_ptr(), w=wd.data_ptr(), bias=bd.data_ptr(), out16=out.ptr + 2 * d, M=batch * mb, N=d, K=kpad, lda=n_mels, Mb=mb,
                                      aBatchStride=stride, ldc=d, cBatchStride=(mb + 2) * d, epi=B.EPI_F16_GELU, scale=1.0)
    what = "conv1 n_mels=%d d=%d %d x 2T=%d" % (n_mels, d, batch, mb)
    report(what, name, fam, wide)
    return fam, wide, out.read(what), what


# 300 tiles of 256 rows: 26 windows of 3000 rows, 383 of 200 (gemmTiled4 needs segments of 256 rows: asked for, gemmTiled8 must take it), 766 of 100 (no lean segmented store)
CONV1_CASES = ([(m, 26, 1500, n) for m in (80, 128) for n in ["t256", "t8-lean", "t8-general", "t4"] + (["t8-lean-mf0", "t8-narrow", "t256-narrow", "t4-narrow"] if m == 80 else [])] +
               [(m, 383, 100, n) for m in (80, 128) for n in ["t256", "t8-lean", "t8-general", "t4"]] +
               [(m, 766, 50, n) for m in (80, 128) for n in ["t256", "t8-lean", "t8-general"]] +
               [(80, 2, 1500, "t128"), (80, 2, 1500, "t128-narrow"), (128, 2, 50, "t128"), (80, 2, 1, "t128")])


@pytest.mark.parametrize("n_mels,batch,T,name", CONV1_CASES)
def test_conv1(n_mels, batch, T, name, gelu_map, golden):
    """lda = n_mels, K = conv1Kpad, segments Mb = 2 T aBatchStride apart; EPI_F16_GELU into padded rows 1 .. 2 T of a second segmented buffer, whose rows 0 and
    2 T + 1 keep the sentinel."""
    d = 128
    flat, w_rows, bias, acc = cached(("conv1", n_mels, batch, T), lambda: conv1_inputs(n_mels, d, batch, T))
    fam, wide, got, what = run_conv1(flat, w_rows, bias, n_mels, T, name)
    same_bits(got, R.epi_conv1(acc, bias, gelu_map), what)
    gelu_within_one_ulp(R.gelu_arg_bits(acc, bias), gelu_map, golden, what)
    want_fam = FAMILIES[name][2] if batch > 2 else B.GEMM_TILED_128
    if want_fam == B.GEMM_TILED4 and 2 * T < 256:
        want_fam = B.GEMM_TILED8
    assert fam == want_fam, (what, name, fam)
    assert wide == expected_wide(fam, name, B.EPI_F16_GELU, Mb=2 * T, segmented=batch > 1), (what, name, wide)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# conv2: stride 2 over conv1's padded output, GELU + the positional row t = m % Mb
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def conv2_inputs(d, batch, T, gaussian=False):
    rng = np.random.default_rng(4000 + d + T + batch)
    ypad = np.zeros((batch, 2 * T + 2, d), np.float16)
    if gaussian:
        ypad[:, 1:-1] = rng.standard_normal((batch, 2 * T, d)).astype(np.float16)
        w_file, bias = (0.05 * rng.standard_normal((d, d, 3))).astype(np.float16), rng.standard_normal(d).astype(np.float32)
    else:
        ypad[:, 1:-1] = R.activations(rng, (batch, 2 * T, d))
        w_file, bias = R.weights(rng, (d, d, 3)), R.biases(rng, d)
    pe = rng.standard_normal((T, d)).astype(np.float32)
    w_rows = R.conv_weight_rows(w_file, 3 * d)
    acc = R.conv_acc(ypad, w_rows, 2)
    return frozen(ypad, w_rows, bias, pe, acc if gaussian else R.as_f32_exact(acc))


def run_conv2(ypad, w_rows, bias, pe, name):
    batch, tp, d = ypad.shape
    T = (tp - 2) // 2
    ad, wd, bd, pd = dev(ypad), dev(w_rows), dev(bias), dev(pe)
    out = Out(batch * T * d, 32)
    with family(name):
        fam, wide = B.op_gemm_encoder(a=ad.data_ptr(), w=wd.data_ptr(), bias=bd.data_ptr(), pe=pd.data_ptr(), out32=out.ptr, M=batch * T, N=d, K=3 * d, lda=2 * d, Mb=T,
                                      aBatchStride=tp * d, ldc=d, epi=B.EPI_CONV2, scale=1.0)
    what = "conv2 d=%d %d x T=%d" % (d, batch, T)
    report(what, name, fam, wide)
    return fam, wide, out.read(what), what


# EPI_CONV2 has no persistent instance and no 256-wide one (gemm_tiled.hip launchTiled): whatever is asked for, the chooser must report gemmTiled's 128-wide tiles
# ("t8-lean" = the default tuning). 52 windows = 78000 rows: 610 tile rows that windows of 1500 rows straddle
CONV2_CASES = ([(52, 1500, n) for n in ("t256", "t256-narrow", "t8-lean")] +
               [(2, T, n) for T in (1500, 375, 1) for n in ["t128"] + (["t128-narrow"] if T == 375 else [])])


@pytest.mark.parametrize("batch,T,name", CONV2_CASES)
def test_conv2(batch, T, name, gelu_map, golden):
    """lda = 2 d (stride 2) over segments of 2 T + 2 padded rows; EPI_CONV2 = float( gelu16( acc + bias ) ) + pe[ m % T ], one FP32 addition."""
    d = 128
    ypad, w_rows, bias, pe, acc = cached(("conv2", batch, T), lambda: conv2_inputs(d, batch, T))
    fam, wide, got, what = run_conv2(ypad, w_rows, bias, pe, name)
    same_bits(got, R.epi_conv2(acc, bias, pe, gelu_map).view(np.uint32), what)
    gelu_within_one_ulp(R.gelu_arg_bits(acc, bias), gelu_map, golden, what)
    assert fam == B.GEMM_TILED_128, (what, name, fam)
    assert wide == expected_wide(fam, name, B.EPI_CONV2), (what, name, wide)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# mel -> conv input
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("rows", [3000, 750, 2])
def test_mel_to_conv_input(n_mels, rows):
    """x16[b][t + 1][c] = fp16( mel[c][off_b + t] ) -- one rounding of an FP32 value: equal bits --, zero where the spectrogram has ended, rows 0 and 2 T + 1 of every
    window untouched. Both forms: offsets into one spectrogram (inside it, straddling its end, beyond it), and per-window descriptors with one null window."""
    rng = np.random.default_rng(n_mels + rows)
    mel_len = 2 * rows + 37
    mel = rng.standard_normal((n_mels, mel_len)).astype(np.float32)
    other = rng.standard_normal((n_mels, rows // 2 + 1)).astype(np.float32)
    stride = (rows + 2) * n_mels + 8
    md, od = dev(mel), dev(other)
    L = B.lib()
    # offsets: window 0 at the start, 1 inside, 2 straddling the end, 3 starting at the end, 4 beyond it
    offs = np.array([0, 17, mel_len - rows // 2 - 1, mel_len, mel_len + 5 * rows], np.int32)
    out = Out(len(offs) * stride, 16)
    B.check(L.wh_op_mel_to_conv_input(None, md.data_ptr(), 0, mel_len, offs.ctypes.data, None, out.ptr, stride, n_mels, rows, len(offs)))
    want = R.mel_to_conv_input([mel] * len(offs), offs, n_mels, rows, stride)
    same_bits(out.read("mel -> conv input, offsets"), want, "mel -> conv input, offsets, n_mels=%d rows=%d" % (n_mels, rows))
    body = want[:, n_mels:(rows + 1) * n_mels].reshape(len(offs), rows, n_mels)
    assert (body[3:] == 0).all() and (body[2, rows // 2 + 1:] == 0).all() and (body[2, :rows // 2 + 1] != 0).any()
    # descriptors: a window of the first spectrogram, a null window (silence), a window of a second, shorter one that ends inside it
    wins = (B.MelWindowC * 3)(B.MelWindowC(md.data_ptr(), mel_len, 5, 0), B.MelWindowC(None, 0, 0, 0), B.MelWindowC(od.data_ptr(), other.shape[1], 1, 0))
    out = Out(3 * stride, 16)
    B.check(L.wh_op_mel_to_conv_input(None, None, 0, 0, None, C.cast(wins, C.c_void_p), out.ptr, stride, n_mels, rows, 3))
    want = R.mel_to_conv_input([mel, None, other], [5, 0, 1], n_mels, rows, stride)
    same_bits(out.read("mel -> conv input, windows"), want, "mel -> conv input, windows, n_mels=%d rows=%d" % (n_mels, rows))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# one Gaussian case per arrangement, default family: a test set that only ever sees dyadic numbers would not notice a kernel that drops low bits
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def fp32_bound(K):
    """test_gpu_ops.py::test_mul_mat's round-off bound of an FP32 sum of K products of magnitude ~0.05"""
    return 2e-5 * max(1.0, np.sqrt(K / 128))


def half_ulp16(x, slack):
    """Half an FP16 unit in the last place at |x| + slack (a value that close to the next binade may round there)."""
    e = np.floor(np.log2(np.maximum(np.abs(x) + slack, 2.0 ** -14)))
    return 2.0 ** (e - 11)


def f16_outputs_close(got_bits, want64, K, what):
    """FP16 outputs of an FP32 value within fp32_bound of want64: half an FP16 ulp of the expected value plus that bound."""
    got = got_bits.view(np.float16).astype(np.float64)
    b = fp32_bound(K)
    err = np.abs(got - want64)
    tol = half_ulp16(want64, b) + b
    print("%s: max error %.3e, largest error / bound %.3f" % (what, err.max(), (err / tol).max()))
    assert (err <= tol).all(), (what, float((err / tol).max()))


def gelu_outputs_between(got_bits, arg64, K, gelu_map, what):
    """gelu16 looks its argument up by its FP16 bits, so an argument within fp32_bound of arg64 gives the map's entry at fp16( arg64 - b ), at fp16( arg64 + b ), or at an
    FP16 number between them -- one and the same entry (then: equal bits) unless the interval straddles a rounding boundary. The map is monotone wherever the
    interval holds more than two FP16 numbers (|arg| < 0.04, far from GELU's minimum at -0.75), so 'between the two ends' says it for all."""
    b = fp32_bound(K)

    def line(u):
        u = u.astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u)
    lo = gelu_map[(arg64 - b).astype(np.float32).astype(np.float16).view(np.uint16)]
    hi = gelu_map[(arg64 + b).astype(np.float32).astype(np.float16).view(np.uint16)]
    l0, l1, g = np.minimum(line(lo), line(hi)), np.maximum(line(lo), line(hi)), line(got_bits)
    print("%s: %.4f of the arguments lie within the FP32 bound of an FP16 rounding boundary" % (what, float((lo != hi).mean())))
    assert ((g >= l0) & (g <= l1)).all(), (what, int(((g < l0) | (g > l1)).sum()))


def test_gaussian_qkv():
    H, M, T = 2, 39000, 1500
    a, w, bias, acc = qkv_inputs(H, M, gaussian=True)
    fam, wide, q, k, v, what = run_qkv(a, w, bias, H, T, "t8-lean")
    assert fam == B.GEMM_TILED8
    x = (acc + bias).reshape(M // T, T, 3, H, 64)
    f16_outputs_close(q, x[:, :, 0].transpose(0, 2, 1, 3).reshape(-1), 64 * H, what + " q, Gaussian")
    f16_outputs_close(k, x[:, :, 1].transpose(0, 2, 1, 3).reshape(-1), 64 * H, what + " k, Gaussian")
    key, dd = np.meshgrid(np.arange(T), np.arange(64), indexing="ij")
    idx = R.v_frag_index(key, dd).ravel()
    vv = v.reshape(M // T, H, -1)
    f16_outputs_close(np.ascontiguousarray(vv[:, :, idx]).reshape(-1), x[:, :, 2].transpose(0, 2, 1, 3).reshape(-1), 64 * H, what + " v, Gaussian")
    live = np.zeros(vv.shape[-1], bool)
    live[idx] = True
    assert (vv[:, :, ~live] == R.SENTINEL16).all()


def test_gaussian_cross_kv():
    H, layers, M, T, b0, cap = 2, 4, 19500, 1500, 2, 16
    a, w, bias, acc = cross_inputs(H, layers, M, gaussian=True)
    fam, wide, k, v, what = run_cross(a, w, bias, H, T, b0, cap, "t8-lean")
    assert fam == B.GEMM_TILED8
    d = 64 * H
    x = acc.reshape(M // T, T, layers, 2, H, 64)
    bb = bias.reshape(layers, 2, H, 64).astype(np.float64)
    wk = (x[:, :, :, 0] * np.float64(np.float32(cross_scale(H)))).transpose(2, 0, 3, 1, 4)          # [layer][b][h][T][64]
    wv = (x[:, :, :, 1] + bb[None, None, :, 1]).transpose(2, 0, 3, 1, 4)
    kk, vv = k.reshape(layers, cap, H, T, 64), v.reshape(layers, cap, H, T, 64)
    f16_outputs_close(np.ascontiguousarray(kk[:, b0:b0 + M // T]).reshape(-1), wk.reshape(-1), d, what + " k, Gaussian")
    f16_outputs_close(np.ascontiguousarray(vv[:, b0:b0 + M // T]).reshape(-1), wv.reshape(-1), d, what + " v, Gaussian")
    for c in (kk, vv):
        assert (c[:, :b0] == R.SENTINEL16).all() and (c[:, b0 + M // T:] == R.SENTINEL16).all()


def test_gaussian_conv1(gelu_map):
    n_mels, d, batch, T = 80, 128, 26, 1500
    flat, w_rows, bias, acc = conv1_inputs(n_mels, d, batch, T, gaussian=True)
    fam, wide, got, what = run_conv1(flat, w_rows, bias, n_mels, T, "t8-lean")
    assert fam == B.GEMM_TILED8
    got = got.reshape(batch, 2 * T + 2, d)
    assert (got[:, 0] == R.SENTINEL16).all() and (got[:, -1] == R.SENTINEL16).all()
    gelu_outputs_between(got[:, 1:-1], acc + bias, w_rows.shape[1], gelu_map, what + ", Gaussian")


def test_gaussian_conv2(gelu_map):
    d, batch, T = 128, 52, 1500
    ypad, w_rows, bias, pe, acc = conv2_inputs(d, batch, T, gaussian=True)
    fam, wide, got, what = run_conv2(ypad, w_rows, bias, pe, "t8-lean")
    assert fam == B.GEMM_TILED_128
    # out = pe + float( g ): g is the FP16 number whose sum with pe rounds to the output; recovered exactly where |g| is not far below |pe|'s last place -- compare
    # instead against the two ends of the interval, each added to pe in FP32 as the kernel does
    b = fp32_bound(3 * d)
    arg = acc + bias
    lo = gelu_map[(arg - b).astype(np.float32).astype(np.float16).view(np.uint16)].view(np.float16).astype(np.float32)
    hi = gelu_map[(arg + b).astype(np.float32).astype(np.float16).view(np.uint16)].view(np.float16).astype(np.float32)
    o = got.view(np.float32).reshape(batch, T, d)
    e0, e1 = (pe[None] + np.minimum(lo, hi)).astype(np.float32), (pe[None] + np.maximum(lo, hi)).astype(np.float32)
    print("%s, Gaussian: %.4f of the arguments lie within the FP32 bound of an FP16 rounding boundary" % (what, float((lo != hi).mean())))
    assert ((o >= e0) & (o <= e1)).all(), int(((o < e0) | (o > e1)).sum())
