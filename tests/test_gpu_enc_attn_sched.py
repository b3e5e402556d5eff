"""GPU: the scheduled tile loop of the one-sweep encoder attention ("enc_sched" 1) against the loop it replaces ("enc_sched" 0).

The scheduled loop moves memory-side latency only (K / V fragment reads ahead of the exponentials, the half-waves' row maximum joined by
v_permlane32_swap, O rescaled in place, sub-tiles wholly beyond T skipped): the arithmetic per query row is the same in the same order, so the
criterion is EQUALITY of the outputs, for "enc_exp" 3 and 5. On Gaussian inputs both loops are also held to test_flash_attention's bounds
against the reference's softmax. Bounded random data almost never takes the rescale branch after a row's first sub-tiles, so a second input
plants late maxima: chosen keys are overwritten with a multiple of a chosen query row, which lifts that row's score at that key more than the
lazy threshold (4) plus a margin of 2 above every earlier score of the row (asserted in numpy).
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import whisper_np as wn  # noqa: E402
from whisper_amd import binding  # noqa: E402

pytestmark = pytest.mark.gpu

D = 64
TILE = 128          # keys per LDS tile of attentionEncW
SUB = 32            # keys per sub-tile (one score MFMA chain)
LAZY = 4.0          # W_LAZY of attn_enc.hip
MARGIN = 2.0


def ptr(t):
    return C.c_void_p(t.data_ptr())


def v_operand(v, T):
    """V in the kernel's operand order (epilogue.h vFragIndex), zero beyond T."""
    BH = v.shape[0]
    Tpad = (T + 255) // 256 * 256
    key, dd = np.meshgrid(np.arange(T), np.arange(D), indexing="ij")
    idx = (((key >> 4) * 2 + (dd >> 5)) * 64 + ((key >> 2) & 1) * 32 + (dd & 31)) * 8 + ((key >> 3) & 1) * 4 + (key & 3)
    vT = np.zeros((BH, D * Tpad), np.float16)
    vT[:, idx.ravel()] = v.reshape(BH, T * D)
    return vT


def run_all(q, k, v, batch, heads, T):
    """{(enc_exp, enc_sched): output} for the one-sweep kernel."""
    qd, kd, vd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (q, k, v_operand(v, T)))
    L = binding.lib()
    res = {}
    try:
        L.wh_debug_set_tuning(binding.TUNE_DEFAULT | binding.TUNE_ATTN_ENC_2SWEEP | binding.TUNE_ATTN_ENC_TABLE | binding.TUNE_ATTN_ENC_TABLE_ANY)
        for exp in (3, 5):
            for sched in (0, 1):
                binding.set_option("enc_exp", exp)
                binding.set_option("enc_sched", sched)
                out = torch.full((batch, T, heads * D), float("nan"), dtype=torch.float16, device="cuda")
                binding.check(L.wh_op_flash_attention(None, ptr(qd), ptr(kd), ptr(vd), ptr(out), batch, heads, T))
                torch.cuda.synchronize()
                res[(exp, sched)] = out.cpu().numpy().astype(np.float32)
    finally:
        L.wh_debug_set_tuning(binding.TUNE_DEFAULT)
        binding.set_option("enc_exp", binding.get_option_default("enc_exp"))
        binding.set_option("enc_sched", binding.get_option_default("enc_sched"))
    return res


def gaussian(batch, heads, T):
    rng = np.random.default_rng(1000 + T)
    q = (rng.standard_normal((batch * heads, T, D)) * 1.5).astype(np.float16)
    k = (rng.standard_normal((batch * heads, T, D)) * 1.5).astype(np.float16)
    v = rng.standard_normal((batch * heads, T, D)).astype(np.float16)
    return q, k, v


def scores(q, k):
    return ((q.astype(np.float32) @ k.astype(np.float32).T) * np.float32(0.125)).astype(np.float32)


SHAPES = [(1, 1, 1), (1, 1, 32), (1, 1, 33), (1, 2, 128), (1, 2, 129), (1, 1, 160), (1, 1, 513), (1, 3, 500), (2, 4, 1500), (1, 1, 1536)]


@pytest.mark.parametrize("batch,heads,T", SHAPES)
def test_gaussian_equal_and_in_bounds(batch, heads, T):
    q, k, v = gaussian(batch, heads, T)
    res = run_all(q, k, v, batch, heads, T)
    want = np.zeros((batch, T, heads * D), np.float32)
    for bh in range(batch * heads):
        P = wn.softmax_table(scores(q[bh], k[bh]))
        want[bh // heads, :, (bh % heads) * D:(bh % heads + 1) * D] = (wn.r16(P) @ v[bh].astype(np.float32)).astype(np.float32)
    want = wn.r16(want)
    for key, got in sorted(res.items()):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print("enc_exp %d enc_sched %d b%d h%d T%d: finite %s, against the reference's softmax max %.3e mean %.3e"
              % (key[0], key[1], batch, heads, T, bool(np.isfinite(got).all()), d.max(), d.mean()))
    for exp in (3, 5):
        print("enc_exp %d: scheduled loop == round-6 loop: %s (%d of %d outputs differ)"
              % (exp, np.array_equal(res[(exp, 0)], res[(exp, 1)]), int((res[(exp, 0)] != res[(exp, 1)]).sum()), res[(exp, 0)].size))
    for key, got in sorted(res.items()):
        assert np.isfinite(got).all(), key
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert d.max() < 6e-3 and d.mean() < 2e-4, key
    for exp in (3, 5):
        assert np.array_equal(res[(exp, 0)], res[(exp, 1)]), exp


def plants_for(T):
    """(query row, key) pairs. A wave of the kernel owns 64 consecutive query rows of a 512-row block as two groups of 32; a lane of the lower
    half-wave holds the keys with key mod 8 < 4 of a sub-tile, the upper half-wave the others."""
    n_tiles = (T + TILE - 1) // TILE
    mid = (n_tiles // 2) * TILE                 # first key of a middle tile (not the last one)
    last_sub = ((T - 1) // SUB) * SUB           # first key of the last sub-tile with a key < T
    p = [(17, 32 + 13),                         # tile 0, sub-tile 1, upper half-wave
         (5, mid + 1),                          # middle tile, sub-tile 0, lower half; wave 0: only its first group raises
         (40, mid + 32 + 5),                    # sub-tile 1, upper half; wave 0: only its second group raises
         (70, mid + 64 + 2), (100, mid + 64 + 14),     # sub-tile 2: both groups of wave 1 raise in the same sub-tile
         (130, mid + 96 + 7),                   # sub-tile 3
         (200, mid + 32 + 3), (200, mid + 64 + 12),    # one row raises in two consecutive sub-tiles
         (333, last_sub),                       # the last valid sub-tile
         (300, T - 1)]                          # the last key
    if T > 512:
        p.append((T - 1, mid + 96 + 20))        # the second query block
    out, seen = [], set()
    for r, j in sorted(p, key=lambda x: x[1]):
        if j not in seen:
            seen.add(j)
            out.append((r, j))
    return out


PLANTED_SHAPES = [(1, 1, 513), (1, 3, 500), (2, 4, 1500), (1, 1, 1536)]


@pytest.mark.parametrize("batch,heads,T", PLANTED_SHAPES)
def test_planted_late_maxima_equal(batch, heads, T):
    q, k, v = gaussian(batch, heads, T)
    plants = plants_for(T)
    assert (T + TILE - 1) // TILE >= 3 and all(r < T and 0 < j < T for r, j in plants)
    for bh in range(batch * heads):
        for r, j in plants:                     # by increasing key: the keys below j are final
            qr = q[bh, r].astype(np.float32)
            earlier = scores(q[bh, r:r + 1], k[bh, :j]).max()
            alpha = (earlier + LAZY + MARGIN + 0.5) * 8.0 / float(qr @ qr)
            k[bh, j] = (alpha * qr).astype(np.float16)
        S = scores(q[bh], k[bh])
        for r, j in plants:
            assert S[r, j] > S[r, :j].max() + LAZY + MARGIN, (bh, r, j, float(S[r, j]), float(S[r, :j].max()))
    assert np.isfinite(k.astype(np.float32)).all()
    res = run_all(q, k, v, batch, heads, T)
    for exp in (3, 5):
        print("planted, enc_exp %d b%d h%d T%d: scheduled loop == round-6 loop: %s (%d of %d outputs differ, max |difference| %.3e)"
              % (exp, batch, heads, T, np.array_equal(res[(exp, 0)], res[(exp, 1)]), int((res[(exp, 0)] != res[(exp, 1)]).sum()), res[(exp, 0)].size,
                 np.abs(res[(exp, 0)] - res[(exp, 1)]).max()))
    for key, got in sorted(res.items()):
        assert np.isfinite(got).all(), key
    for exp in (3, 5):
        assert np.array_equal(res[(exp, 0)], res[(exp, 1)]), exp
