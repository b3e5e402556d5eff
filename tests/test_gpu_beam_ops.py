"""GPU tests of the beam step's kernels at op level and of configs[2] (large-v2, 8 windows x 5 hypotheses, 50 forced steps) at its own size.

  * the decoder's vocabulary softmax (wh_op_vocab_soft_max): softMaxRowsReg (option beam_regs 1, up to 52224 columns) and softMaxRows (beam_regs 0,
    and every width beyond) against the float64 table softmax, and against each other bit for bit;
  * wh_op_sample_best / wh_op_beam_candidates against oracle sample_best / beam_candidates, on rows built to hit each of sampleBest's rules;
  * wh_op_reorder_self_cache: reorderCacheGroup<G> for G = 2 .. 8 and the two-phase copy against a numpy gather and against each other;
  * the whole ranked beam step on the large-v2 shape: device ranking == host ranking, every round-6 option off == on, cross_mfma 0 against 1 within a
    measured band, two runs identical.
Options are process-global and captured into graphs: every test sets them before it creates a context and restores them in `finally`.
"""
import ctypes as C
import time
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import whisper_np as wn  # noqa: E402
from whisper_amd import binding, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

VOCABS = (51864, 51865, 51866)
TOKEN_DT = np.dtype([("id", "<i4"), ("tid", "<i4"), ("p", "<f4"), ("pt", "<f4"), ("ptsum", "<f4")])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr())


class options:
    """with options(beam_regs=0, ...): library options for the duration of a block, restored from binding.OPTION_DEFAULTS."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            binding.set_option(k, v)

    def __exit__(self, *a):
        for k in self.kw:
            binding.set_option(k, binding.OPTION_DEFAULTS[k])


# ---------------------------------------------------------------------------------------------------------------------
# vocabulary softmax
# ---------------------------------------------------------------------------------------------------------------------
def _softmax_rows(rows, cols, seed):
    """Rows of five kinds: -inf entries, the maximum in the partial last 1024-chunk, one finite entry, logits of size +-80, plain logits."""
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal((rows, cols))).astype(np.float32)
    for r in range(rows):
        kind = (r + cols) % 5
        if kind == 0:
            x[r, rng.integers(0, cols, max(1, cols // 7))] = -np.inf
            x[r, rng.integers(0, cols)] = 1.0                                     # at least one finite entry
        elif kind == 1:
            x[r, cols - 1] = 40.0                                                 # the last column: the partial chunk of the row
        elif kind == 2:
            x[r] = -np.inf
            x[r, rng.integers(0, cols)] = -3.0
        elif kind == 3:
            x[r] = rng.uniform(-80.0, 80.0, cols).astype(np.float32)
    return x


@pytest.mark.parametrize("cols", [1, 7, 1024, 1025, 51864, 51865, 51866, 52224, 52225])
def test_vocab_soft_max_both_kernels(cols):
    """launchVocabSoftMax, the decoder's own route: softMaxRowsReg (beam_regs 1; the row in registers, SC_PER * 1024 = 52224 columns at most) and
    softMaxRows (beam_regs 0; 52225 columns take it whatever the option) give the same bits, and both stay within test_soft_max's bound of the
    float64 table softmax (exp16 of the same FP16 argument, one FP16 ulp where expf and glibc round differently)."""
    L = binding.lib()
    for rows in (1, 5, 40, 128):
        x = _softmax_rows(rows, cols, rows * 100003 + cols)
        want = wn.softmax_table(x)
        xd = dev(x)
        got = {}
        for regs in (1, 0):
            out = torch.full((rows, cols), float("nan"), dtype=torch.float32, device="cuda")
            with options(beam_regs=regs):
                binding.check(L.wh_op_vocab_soft_max(None, ptr(xd), ptr(out), rows, cols))
                torch.cuda.synchronize()
            got[regs] = out.cpu().numpy()
        assert np.array_equal(got[1].view(np.uint32), got[0].view(np.uint32)), (rows, cols, "softMaxRowsReg and softMaxRows differ")
        assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32)), "the input was written"
        g = got[1]
        assert np.isfinite(g).all() and (g[np.isneginf(x)] == 0.0).all()
        d = np.abs(g.astype(np.float64) - want.astype(np.float64))
        print("vocab soft_max %3d x %5d: maxdiff %.3e, %d of %d differ" % (rows, cols, d.max(), int((d > 0).sum()), d.size))
        assert d.max() < 1e-3 * want.max() and (d > 0).mean() < 0.01


# ---------------------------------------------------------------------------------------------------------------------
# sampler and beam candidates
# ---------------------------------------------------------------------------------------------------------------------
def _sampler_rows(V, sp, seed):
    """Probability rows (not normalised; powers of two, so that every double sum is exact in any order) that hit each of sampleBest's rules.
    Returns [(name, row)]."""
    beg, sot, solm, tnot = sp["beg"], sp["sot"], sp["solm"], sp["not_"]
    rng = np.random.default_rng(seed)

    def background():
        """small powers of two on text tokens only, so that the timestamp mass is exactly what a row sets"""
        r = np.zeros(V, np.float32)
        idx = rng.integers(0, beg, 3000)
        r[idx] = np.float32(2.0) ** -rng.integers(20, 40, len(idx)).astype(np.float32)
        return r

    rows = []
    r = background()
    r[[100, 101]] = [2.0 ** -4, 2.0 ** -5]
    r[beg + 5], r[beg + 700] = 2.0 ** -3, 2.0 ** -6                            # timestamp mass above the best text token
    rows.append(("ts_above", r))
    r = background()
    r[200] = 2.0 ** -2
    r[beg + 1], r[beg + 2] = 2.0 ** -3, 2.0 ** -3                              # timestamp mass EQUAL to the best text token: text stays
    rows.append(("ts_equal", r))
    r = background()
    r[300] = 2.0 ** -2
    r[beg + 40], r[beg + 1200] = 2.0 ** -4, 2.0 ** -5                          # below
    rows.append(("ts_below", r))
    r = background()
    r[400] = 2.0 ** -3
    r[beg + 150], r[beg + 100], r[beg + 101], r[beg + 20] = 2.0 ** -1, 2.0 ** -3, 2.0 ** -2, 2.0 ** -4   # best timestamps above beg + 100
    rows.append(("initial_cap", r))
    for k in (1, 2, 3):                                                         # sot / solm / not as the top 1, 2, 3 tokens
        r = background()
        for j, s in enumerate((sot, solm, tnot)[:k]):
            r[s] = 2.0 ** -(1 + j)
        r[500], r[501] = 2.0 ** -5, 2.0 ** -6
        rows.append(("specials_top%d" % k, r))
    r = background()
    r[[7, 7 + 1024, 7 + 2048, 7 + 5 * 1024, 1030]] = 2.0 ** -3              # exact ties across the 1024-thread stride
    r[beg + 3], r[beg + 3 + 1024] = 2.0 ** -5, 2.0 ** -5
    rows.append(("ties_text", r))
    r = background()
    r[[beg + 3, beg + 3 + 1024, beg + 4]] = 2.0 ** -2                         # ties among the timestamps, which win by mass
    r[9] = 2.0 ** -3
    rows.append(("ties_ts", r))
    r = wn.softmax_table((3.0 * rng.standard_normal(V)).astype(np.float32)[None, :])[0]
    rows.append(("softmax", r))
    return rows


def _run_tokens(fn, probs_dev, rows, V, sp, force, initial, width=None):
    out = torch.zeros(rows * (width or 1) * 5, dtype=torch.int32, device="cuda")
    args = [None, ptr(probs_dev), rows, V, sp["beg"], sp["sot"], sp["solm"], sp["not_"], int(force), int(initial)]
    args += [width] if width else []
    binding.check(fn(*args, ptr(out)))
    torch.cuda.synchronize()
    return np.frombuffer(out.cpu().numpy().tobytes(), TOKEN_DT).reshape(rows, width or 1)


def _assert_same(got, want, where):
    assert [int(x) for x in got["id"]] == [w["id"] for w in want], where
    assert [int(x) for x in got["tid"]] == [w["tid"] for w in want], where
    assert np.array_equal(got["p"], np.asarray([w["p"] for w in want], np.float32)), where
    for k in ("pt", "ptsum"):
        assert np.allclose(got[k], [w[k] for w in want], rtol=1e-6, atol=0), (where, k)


@pytest.mark.parametrize("V", VOCABS)
def test_sample_best_and_beam_candidates_against_the_oracle(V):
    """wh_op_sample_best and wh_op_beam_candidates (widths 1 .. 8) against oracle sample_best / beam_candidates on rows built for each rule: timestamp
    mass above / equal to / below the best text token, forceTimestamp, isInitial with the best timestamps above beg + 100, sot / solm / not as the
    top 1 .. 3 tokens, exact ties across the 1024-thread stride, an all-NaN row (the ids stay in range), and a vocabulary of beg + 3 tokens where
    fewer than `width` survive. Ids and p equal, pt / ptsum within 1e-6 relative."""
    sp = gf.special_tokens(SimpleNamespace(n_vocab=V))
    L = binding.lib()
    named = _sampler_rows(V, sp, V)
    probs = np.stack([r for _, r in named] + [np.full(V, np.nan, np.float32)])
    pd = dev(probs)
    small_V = sp["beg"] + 3
    small = np.stack([named[0][1][:small_V], named[2][1][:small_V]])
    sd = dev(small)
    n = len(named)
    for force in (False, True):
        for initial in (False, True):
            for mat, md, nv in ((probs, pd, V), (small, sd, small_V)):
                rows = mat.shape[0]
                want = [wn.beam_candidates(mat[i], sp["beg"], sp["sot"], sp["solm"], sp["not_"], force, initial, width=8) for i in range(rows)]
                sb = _run_tokens(L.wh_op_sample_best, md, rows, nv, sp, force, initial)
                for width in range(1, 9):
                    got = _run_tokens(L.wh_op_beam_candidates, md, rows, nv, sp, force, initial, width)
                    for i in range(rows):
                        where = (nv, force, initial, width, named[i][0] if nv == V and i < n else ("nan" if nv == V else "small%d" % i))
                        if nv == V and i == n:
                            assert ((got["id"][i] >= 0) & (got["id"][i] < nv)).all() and 0 <= sb["id"][i, 0] < nv, where
                            continue
                        _assert_same(got[i], want[i][:width], where)
                        if width == 1:
                            _assert_same(sb[i], want[i][:1], where + ("sample_best",))
    # the rows meet the rules they were built for
    pick = lambda i, f=False, ini=False: wn.sample_best(probs[i], sp["beg"], sp["sot"], sp["solm"], sp["not_"], f, ini)["id"]
    names = [nm for nm, _ in named]
    assert pick(names.index("ts_above")) == sp["beg"] + 5 and pick(names.index("ts_equal")) == 200 and pick(names.index("ts_below")) == 300
    assert pick(names.index("ts_below"), True) == sp["beg"] + 40 and pick(names.index("initial_cap"), False, True) == sp["beg"] + 100
    assert pick(names.index("specials_top3")) == 500 and pick(names.index("ties_text")) == 7 and pick(names.index("ties_ts")) == sp["beg"] + 3


# ---------------------------------------------------------------------------------------------------------------------
# self-attention cache reorder
# ---------------------------------------------------------------------------------------------------------------------
KEY_STRIDE = 448


def _parents(G, windows):
    """Window w of the batch: identity, a cycle, a fan-out from one parent, a full reversal, identity again (absolute indices)."""
    local = [np.arange(G), (np.arange(G) + 1) % G, np.full(G, G // 2), G - 1 - np.arange(G), np.arange(G)]
    return np.concatenate([local[w % len(local)] + w * G for w in range(windows)]).astype(np.int32)


def _reorder(cache0, parents, rows_dev, layers, S, heads, group):
    """One wh_op_reorder_self_cache on copies of cache0 (K and V the same start, V with the sign bit flipped); returns (K, V) after the move."""
    k, v = cache0.clone(), _flip(cache0)
    sk, sv = torch.empty_like(k), torch.empty_like(v)
    pd, rd = dev(parents), dev(rows_dev)
    binding.check(binding.lib().wh_op_reorder_self_cache(None, ptr(k), ptr(v), ptr(sk), ptr(sv), ptr(pd), ptr(rd), layers, S, S, heads, KEY_STRIDE, group))
    torch.cuda.synchronize()
    return k, v


def _flip(x):
    """x with every sign bit flipped, NaN payloads kept (bit operations only)."""
    return (x.view(torch.int16) ^ -32768).view(torch.float16)


def _sentinel(cache, rows_dev):
    """Rows at and beyond rows_dev[j] of sequence j: a quiet NaN whose payload is j, so that a row copied from another sequence shows."""
    for j in range(cache.shape[1]):
        cache.view(torch.int16)[:, j, :, min(max(int(rows_dev[j]), 0), KEY_STRIDE):] = 0x7E00 | (j + 1)


def _gather(cache0, parents, rows_dev):
    """numpy's answer: rows [0, min(max(rows, 0), keyStride)) of sequence j are those of parents[j]; every other element as it was."""
    want = cache0.clone()
    for j, p in enumerate(parents):
        r = min(max(int(rows_dev[j]), 0), KEY_STRIDE)
        if p != j and r:
            want[:, j, :, :r] = cache0[:, p, :, :r]
    return want


@pytest.mark.parametrize("heads", [6, 20])
@pytest.mark.parametrize("G", [2, 3, 4, 5, 6, 7, 8])
def test_reorder_self_cache_group_kernel(G, heads):
    """reorderCacheGroup<G> (reorder_group 1) and the two-phase copy (reorder_group 0) against a numpy gather, bit for bit: 2 layers, 5 windows
    (identity, cycle, fan-out, reversal, identity), rows 0 / 1 / 447 / 448 / 1000 (clamped to keyStride) rotated over the windows. Rows at and
    beyond `rows` hold a NaN sentinel whose payload names the sequence, so a kernel that copied more rows than `rows` would show; they stay as they
    were, and so does every window whose parents are the identity."""
    layers, windows = 2, 5
    S = G * windows
    parents = _parents(G, windows)
    g = torch.Generator(device="cuda").manual_seed(G * 100 + heads)
    base = torch.randn((layers, S, heads, KEY_STRIDE, 64), generator=g, device="cuda").half()
    ident = [w for w in range(windows) if (parents[w * G:(w + 1) * G] == np.arange(w * G, (w + 1) * G)).all()]
    for rot in range(5):
        wrows = np.roll(np.array([0, 1, 447, 448, 1000]), rot)
        rows_dev = np.repeat(wrows, G).astype(np.int32)
        cache0 = base.clone()
        _sentinel(cache0, rows_dev)
        want = _gather(cache0, parents, rows_dev)
        got = {}
        for grp in (1, 0):
            with options(reorder_group=grp):
                got[grp] = _reorder(cache0, parents, rows_dev, layers, S, heads, G)
        for grp in (1, 0):
            k, v = got[grp]
            assert torch.equal(k.view(torch.int16), want.view(torch.int16)), (G, heads, rot, grp, "K")
            assert torch.equal(v.view(torch.int16), _flip(want).view(torch.int16)), (G, heads, rot, grp, "V")
        for w in ident:
            assert torch.equal(got[1][0][:, w * G:(w + 1) * G].view(torch.int16), cache0[:, w * G:(w + 1) * G].view(torch.int16))


def test_reorder_self_cache_two_phase_when_the_batch_is_not_a_multiple_of_the_group():
    """sequences % group != 0: the two-phase copy through the scratch cache, whatever reorder_group says; parents may cross group boundaries
    (any permutation or fan-out inside the batch), rows per sequence from rowsDev, clamped."""
    layers, heads, S, group = 2, 20, 23, 5
    rng = np.random.default_rng(5)
    parents = rng.permutation(S).astype(np.int32)
    parents[[3, 4, 17]] = parents[10]                                             # a fan-out on top of a permutation
    parents[[0, 11]] = [0, 11]                                                    # and two that stay
    rows_dev = rng.choice([0, 1, 447, 448, 1000, 100], S).astype(np.int32)
    g = torch.Generator(device="cuda").manual_seed(23)
    cache0 = torch.randn((layers, S, heads, KEY_STRIDE, 64), generator=g, device="cuda").half()
    _sentinel(cache0, rows_dev)
    want = _gather(cache0, parents, rows_dev)
    for grp in (1, 0):
        with options(reorder_group=grp):
            k, v = _reorder(cache0, parents, rows_dev, layers, S, heads, group)
        assert torch.equal(k.view(torch.int16), want.view(torch.int16)) and torch.equal(v.view(torch.int16), _flip(want).view(torch.int16)), grp


def test_beam_ops_reject_bad_sizes():
    """The host rejects what the kernels cannot do, before anything is launched."""
    L = binding.lib()
    x = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = ptr(x)
    assert L.wh_op_vocab_soft_max(None, p, p, 0, 8) != 0 and L.wh_op_vocab_soft_max(None, p, p, 1, 0) != 0
    assert L.wh_op_sample_best(None, p, 1, 8, 8, 1, 2, 3, 0, 0, p) != 0                     # no timestamp token
    assert L.wh_op_beam_candidates(None, p, 1, 16, 8, 1, 2, 3, 0, 0, 9, p) != 0              # width 9
    assert L.wh_op_beam_candidates(None, p, 1, 16, 8, 1, 2, 3, 0, 0, 0, p) != 0
    assert L.wh_op_beam_candidates(None, p, 1, 16, 8, 1, 9, 3, 0, 0, 2, p) != 0              # a special among the timestamps
    assert L.wh_op_reorder_self_cache(None, p, p, p, p, p, p, 1, 4, 3, 1, 8, 2) != 0         # sequences > maxSeq
    assert L.wh_op_reorder_self_cache(None, p, p, p, p, p, p, 1, 4, 4, 1, 8, 0) != 0         # group 0
    assert L.wh_op_reorder_self_cache(None, p, p, p, p, p, None, 1, 4, 4, 1, 8, 2) != 0      # no rows


# ---------------------------------------------------------------------------------------------------------------------
# configs[2] at its own size: large-v2, 8 windows x 5 hypotheses, 50 forced steps
# ---------------------------------------------------------------------------------------------------------------------
WINDOWS, HYP, N_STEPS = 8, 5, 50
# cross_mfma 0 against 1 along the cross_mfma 1 search, teacher-forced: |delta log p| of the 2040 selected tokens. Measured on the MI355X: max 3.53e-3,
# mean 7.78e-4; survivors compared at 331 of 408 (window, step) pairs. The bounds are 2 x the measured figures (rounded down).
DLOGP_MAX, DLOGP_MEAN = 7.0e-3, 1.5e-3
ROUND6_OFF = dict(beam_regs=0, reorder_group=0, vocab_lds=0, dec_split=0, dec_lds=0, dec_lds_ks=1)


@pytest.fixture(scope="module")
def large_v2():
    model = gf.synth_model("large-v2", seed=1)
    hp = model.hparams
    m = binding.HipModel.from_ggml(model)
    del model
    sp = gf.special_tokens(hp)
    mels = []
    for i in range(WINDOWS):                                                        # bench.py run_chunks' synthetic chunks
        g = torch.Generator(device="cuda").manual_seed(1000 + i)
        mels.append(torch.rand((hp.n_mels, 3000), generator=g, device="cuda") * 2.0 - 1.0)
    prompt = np.asarray([sp["sot"], sp["sot"] + 1, sp["transcribe"]], np.int32)
    yield SimpleNamespace(m=m, hp=hp, mel=torch.stack(mels), prompt=prompt)
    m.close()


def _logp(p):
    return np.log(np.maximum(np.asarray(p, np.float64), 1e-30))


def _host_ranked(c, L2, probs=False):
    """The search ranked on the host after every step (wh_beam_candidates -> numpy: parent score + log p, stable order -> wh_reorder_self_cache),
    as test_gpu_model.test_beam_search_steps_on_the_device does. Returns the chains [w][j][steps + 1], the scores and per step what was fed
    (parents, tokens) with the candidates (width HYP + 1: the sixth is the best excluded continuation of each parent) and, with `probs`, the rows."""
    k, hyp, S, nb = WINDOWS, HYP, WINDOWS * HYP, len(L2.prompt)
    c.encode(L2.mel)
    _, pr = c.decode(np.tile(L2.prompt, (S, 1)), 0, want_logits=False, want_probs=probs)
    steps = [dict(parents=None, tokens=None, cand=c.beam_candidates(S, hyp + 1, True, True), probs=pr)]
    cand = steps[0]["cand"]
    tok = cand["id"][::hyp, :hyp].astype(np.int32)
    score = _logp(cand["p"][::hyp, :hyp])
    parents = (np.arange(k)[:, None] * hyp + np.zeros((1, hyp), np.int64)).astype(np.int32)
    steps[0].update(par_local=np.zeros((k, hyp), np.int64), order=np.arange(hyp)[None, :].repeat(k, 0))
    hist = tok[:, :, None]
    for s_ in range(N_STEPS):
        c.reorder_self_cache(parents.reshape(-1), nb + s_)
        _, pr = c.decode(tok.reshape(-1, 1), nb + s_, want_logits=False, want_probs=probs)
        cand6 = c.beam_candidates(S, hyp + 1)
        cand = {key: v[:, :hyp] for key, v in cand6.items()}
        pool = score[:, :, None] + _logp(cand["p"].reshape(k, hyp, hyp))
        flat = pool.reshape(k, hyp * hyp)
        order = np.argsort(-flat, axis=1, kind="stable")[:, :hyp]
        steps.append(dict(parents=parents.reshape(-1).copy(), tokens=tok.reshape(-1).copy(), cand=cand6, probs=pr, par_local=order // hyp, order=order,
                          score_before=score.copy()))
        par_local = order // hyp
        score = np.take_along_axis(flat, order, axis=1)
        tok = np.take_along_axis(cand["id"].reshape(k, hyp * hyp), order, axis=1).astype(np.int32)
        parents = (np.arange(k)[:, None] * hyp + par_local).astype(np.int32)
        hist = np.concatenate([np.take_along_axis(hist, par_local[:, :, None], axis=1), tok[:, :, None]], axis=2)
    return hist, score, steps


def _device_ranked(c, L2):
    c.encode(L2.mel)
    c.beam_window_start(np.tile(L2.prompt, (WINDOWS, 1)), HYP, N_STEPS)
    st = c.beam_window_status()
    rec = c.beam_window_records(0, N_STEPS + 1)
    chains = [[c.beam_chain(rec, w, st[w]["live"][j]["rec"]) for j in range(st[w]["nLive"])] for w in range(WINDOWS)]
    sums = np.array([[st[w]["live"][j]["sum"] for j in range(st[w]["nLive"])] for w in range(WINDOWS)])
    return st, rec, chains, sums


def test_configs2_device_ranking_options_and_repeatability(large_v2):
    """(a) the device-ranked search (wh_beam_window_*: reorderCacheGroup<5>, 20 heads x 32 layers) == the host-ranked one (the two-phase copy): chains identical,
    scores within 1e-9; (d) a second device-ranked run gives identical records, every score is finite and is the sum of its chain's log p, which never
    increases along the chain; (b) with beam_regs, reorder_group, vocab_lds, dec_split, dec_lds 0 and dec_lds_ks 1 the device-ranked chains and scores are the
    same bits as with the defaults."""
    L2 = large_v2
    t0 = time.perf_counter()
    c = binding.HipContext(L2.m, WINDOWS, hypotheses=HYP)
    try:
        hist, score, _ = _host_ranked(c, L2)
        st, rec, chains, sums = _device_ranked(c, L2)
        for w in range(WINDOWS):
            assert st[w]["step"] == N_STEPS + 1 and st[w]["nLive"] == HYP and st[w]["nFinished"] == 0 and not st[w]["done"]
            for j in range(HYP):
                assert chains[w][j] == [int(x) for x in hist[w, j]], (w, j)
                assert abs(sums[w, j] - score[w, j]) < 1e-9 * max(1.0, abs(score[w, j])), (w, j)
        st2, rec2, chains2, sums2 = _device_ranked(c, L2)
        assert rec2.tobytes() == rec.tobytes() and chains2 == chains and np.array_equal(sums2, sums)
        assert np.isfinite(sums).all()
        for w in range(WINDOWS):
            for j in range(HYP):
                r, lp = st[w]["live"][j]["rec"], []
                while r >= 0:
                    e = rec[r // HYP, w, r % HYP]
                    lp.append(float(_logp(e["p"])))
                    r = int(e["parent"])
                cum = np.cumsum(lp[::-1])
                assert np.isfinite(cum).all() and (np.diff(cum) <= 0).all() and abs(cum[-1] - sums[w, j]) < 1e-9 * max(1.0, abs(sums[w, j]))
    finally:
        c.close()
    with options(**ROUND6_OFF):
        c = binding.HipContext(L2.m, WINDOWS, hypotheses=HYP)
        try:
            _, _, chains0, sums0 = _device_ranked(c, L2)
        finally:
            c.close()
    assert chains0 == chains, "the round-6 options change the chains"
    assert np.array_equal(sums0, sums), ("the round-6 options change the scores", float(np.abs(sums0 - sums).max()))
    print("configs[2] at its size: device == host ranking, round-6 options off == on, two runs identical; best scores %s; %.1f s" %
          (np.round(sums.max(axis=1), 3), time.perf_counter() - t0))


def test_configs2_cross_attention_on_the_matrix_cores(large_v2):
    """(c) cross_mfma 1 (attentionDecM, the default) against cross_mfma 0 (attentionDecG): the cross_mfma 1 host-ranked search is replayed with cross_mfma 0,
    teacher-forced (its parents and tokens), and the probabilities of the selected tokens compared: |delta log p| within the committed band. Survivors:
    the band of a (window, step) is the largest |delta| of parent score + log p over every token either setting proposes (cross_mfma 1's HYP + 1
    candidates per parent, cross_mfma 0's HYP), parent scores accumulated along the chain. Where both settings apply the same mask to every parent (the
    timestamp-vs-text decision of sampleBest) and the gap between the 5th survivor and the best continuation cross_mfma 1 excludes exceeds twice the band,
    every token cross_mfma 0 could rank is within the band of its cross_mfma 1 value and below the gap -- so cross_mfma 0 must rank the same survivors.
    Measured: |delta log p| max 3.53e-3, mean 7.78e-4 (the bounds DLOGP_MAX / DLOGP_MEAN are twice
    that); the test prints at how many (window, step) pairs the survivors were compared."""
    L2 = large_v2
    t0 = time.perf_counter()
    k, hyp, S, nb = WINDOWS, HYP, WINDOWS * HYP, len(L2.prompt)
    c = binding.HipContext(L2.m, WINDOWS, hypotheses=HYP)
    try:
        _, _, steps = _host_ranked(c, L2, probs=True)
    finally:
        c.close()
    beg = gf.special_tokens(L2.hp)["beg"]

    def only_ts(p):
        """sampleBest's decision per row (not the first step's, which forces timestamps): the timestamp mass above the best text token"""
        return p[:, beg:].astype(np.float64).sum(axis=1) > np.maximum(p[:, :beg].max(axis=1), -1.0)

    dl, checked, total, flips = [], 0, 0, 0
    with options(cross_mfma=0):
        c = binding.HipContext(L2.m, WINDOWS, hypotheses=HYP)
        try:
            c.encode(L2.mel)
            score0 = np.zeros((k, hyp))
            for s_, st in enumerate(steps):
                if s_ == 0:
                    _, pr = c.decode(np.tile(L2.prompt, (S, 1)), 0, want_logits=False)
                    cand0 = c.beam_candidates(S, hyp, True, True)
                    rows_of = lambda w: np.full(hyp, w * hyp)                       # the first ranking: every slot holds the prompt, slot 0 speaks
                    base0, base1 = np.zeros((k, hyp)), np.zeros((k, hyp))
                else:
                    c.reorder_self_cache(st["parents"], nb + s_ - 1)
                    _, pr = c.decode(st["tokens"][:, None], nb + s_ - 1, want_logits=False)
                    cand0 = c.beam_candidates(S, hyp)
                    rows_of = lambda w: w * hyp + np.arange(hyp)
                    base0, base1 = score0, st["score_before"]
                c6, pr1 = st["cand"], st["probs"]
                new0 = np.zeros((k, hyp))
                for w in range(k):
                    src = rows_of(w) if s_ else rows_of(w)[:1]
                    n_par = len(src)
                    ids1 = c6["id"][src].astype(np.int64)                            # [parents][hyp + 1]
                    v1 = base1[w, :n_par, None] + _logp(c6["p"][src])
                    v0 = base0[w, :n_par, None] + _logp(pr[src[:, None], ids1])
                    ids0 = cand0["id"][src].astype(np.int64)                         # [parents][hyp]: what cross_mfma 0 proposes
                    band = max(float(np.abs(v0 - v1).max()),
                               float(np.abs(_logp(cand0["p"][src]) - _logp(pr1[src[:, None], ids0]) + base0[w, :n_par, None] - base1[w, :n_par, None]).max()))
                    same_mask = s_ == 0 or np.array_equal(only_ts(pr[src]), only_ts(pr1[src]))
                    flips += not same_mask
                    pool1 = v1[:, :hyp].reshape(-1)
                    o1 = np.argsort(-pool1, kind="stable")
                    sel = o1[:hyp]
                    assert s_ == 0 or np.array_equal(sel, st["order"][w])
                    contender = max(float(pool1[o1[hyp]]) if len(o1) > hyp else -np.inf, float(v1[:, hyp].max()))
                    gap = float(pool1[sel[-1]]) - contender
                    d = (v0[:, :hyp].reshape(-1) - pool1)[sel] - (base0[w, sel // hyp] - base1[w, sel // hyp] if s_ else 0.0)
                    dl.extend(np.abs(d).tolist())
                    new0[w] = v0[:, :hyp].reshape(-1)[sel]
                    total += 1
                    if same_mask and gap > 2.0 * band:
                        checked += 1
                        pool0 = (base0[w, :n_par, None] + _logp(cand0["p"][src])).reshape(-1)
                        o0 = np.argsort(-pool0, kind="stable")[:hyp]
                        same = {(int(i // hyp), int(ids0[i // hyp, i % hyp])) for i in o0} == \
                               {(int(i // hyp), int(ids1[i // hyp, i % hyp])) for i in sel}
                        assert same, ("cross_mfma 0 ranks other survivors", s_, w, gap, band)
                score0 = new0
        finally:
            c.close()
    dl = np.asarray(dl)
    print("configs[2] cross_mfma 0 vs 1, teacher-forced along the cross_mfma 1 search: |delta log p| of the selected tokens max %.3e mean %.3e over %d; "
          "survivors compared at %d of %d (window, step) pairs (%d with a mask that differs); %.1f s" % (dl.max(), dl.mean(), len(dl), checked, total, flips,
                                                                                            time.perf_counter() - t0))
    assert dl.max() < DLOGP_MAX and dl.mean() < DLOGP_MEAN
    assert checked > total // 2, "too few steps with a clear gap: the survivor check says little"
