"""GPU tests of scoring a given transcript ("Scoring").

  * wh_op_token_scores against the float64 restatement (tests/token_score_ref.py): both forms of the kernel, strides, guards, every kind of target;
  * wh_score_tokens against the two oracles (tests/golden/ref_score_d128.json, written on the CPU by tests/golden/make_golden_score.py);
  * the records do not depend on the chunk size (bit for bit) and move within the yardstick with the batch;
  * a corrupted transcript scores lower; nothing else of the context moves; the refusals.
The CPU twin: tests/test_score_cpu.py."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import token_score_ref as TS  # noqa: E402
from whisper_amd import binding  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, GOLDEN)
import make_golden_score as mk  # noqa: E402

REC = binding.TOKEN_SCORE_DTYPE
SC_REG_MAX = 51 * 1024                                                           # the longest row tokenScoreKernel keeps in registers


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


class options:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            binding.set_option(k, v)

    def __exit__(self, *a):
        for k in self.kw:
            binding.set_option(k, binding.OPTION_DEFAULTS[k])


# ---------------------------------------------------------------------------------------------------------------------
# 1. the op
# ---------------------------------------------------------------------------------------------------------------------
G = 4096                                                                         # guard band before and behind the rows (floats) and the records
SENTINEL = 0x5A5A5A5A
KINDS = ("id 0", "id V - 1", "the arg-max", "the higher id of a tied maximum", "a tie with a lower id", "a target at -inf")
# logprob / bestLogprob against float64, where both are finite. Derived, not measured: the sum is double over terms whose FP32 expf carries a few ulps
# (<= 2.4e-7 relative, hence <= 2.4e-7 absolute behind the logarithm); the result is rounded once to float, half an ulp of a magnitude below 64 = 3.8e-6.
TOL = 1e-5


def _rows(rows, V, seed, first_kind=0):
    """Seeded logits with -inf entries; row r's target is of kind KINDS[(first_kind + r) % 6]."""
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal((rows, V))).astype(np.float32)
    t = np.zeros(rows, np.int32)
    for r in range(rows):
        x[r, rng.integers(0, V, V // 9)] = -np.inf
        kind = (first_kind + r) % 6
        a, b = sorted(int(v) for v in rng.choice(V, 2, replace=False))
        if kind == 0:
            t[r] = 0
        elif kind == 1:
            t[r] = V - 1
        elif kind == 2:
            x[r, b] = 14.5 if r % 2 else x[r, b]                                 # a peaked row and a flat one
            t[r] = int(np.argmax(x[r]))
        elif kind == 3:
            x[r, a] = x[r, b] = np.float32(x[r].max() + 1.5)
            t[r] = b
        elif kind == 4:
            x[r, a] = x[r, b] = np.float32(1.25)
            t[r] = b
        else:
            x[r, a] = -np.inf
            t[r] = a
    return x, t


def _run_op(x, t, stride=None):
    """The op on rows `stride` floats apart, NaN in front of, between and behind them, the records between sentinels. Returns the records; asserts that nothing
    else was written."""
    rows, V = x.shape
    stride = V if stride is None else stride
    flat = np.full(G + rows * stride + G, np.nan, np.float32)
    for r in range(rows):
        flat[G + r * stride:G + r * stride + V] = x[r]
    xd, td = dev(flat), dev(t)
    out = torch.full(((G + rows + G) * 4,), SENTINEL, dtype=torch.int32, device="cuda")
    binding.op_token_scores(ptr(xd, 4 * G), stride, rows, V, ptr(td), ptr(out, 16 * G))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:4 * G] == SENTINEL).all() and (got[4 * (G + rows):] == SENTINEL).all(), "a record outside the destination was written"
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), flat.view(np.uint32)), "the input was written"
    return got[4 * G:4 * (G + rows)].copy().view(REC)


def _check(got, x, t, note):
    want = TS.score_rows(x, t)
    assert np.array_equal(got["best"], want["best"]), (note, "best", got["best"], want["best"])
    assert np.array_equal(got["rank"], want["rank"]), (note, "rank", got["rank"], want["rank"])
    worst = 0.0
    for k in ("logprob", "bestLogprob"):
        g, w = got[k].astype(np.float64), want[k]
        fin = np.isfinite(w)
        assert np.array_equal(np.isneginf(g), np.isneginf(w)) and np.isfinite(g[fin]).all(), (note, k, g, w)
        if fin.any():
            worst = max(worst, float(np.abs(g[fin] - w[fin]).max()))
    print("%s: largest |logprob - float64| %.2e (bound %.0e)" % (note, worst, TOL))
    assert worst <= TOL, (note, worst)
    assert np.isfinite(want["bestLogprob"]).all()


@pytest.mark.parametrize("rows", [1, 3, 65])
@pytest.mark.parametrize("V", [1000, 51865, 51866, 52300])
def test_op_against_the_float64_restatement(V, rows):
    """51865 and 51866 take the register form, 52300 (above 51 x 1024) the two-read form, 1000 a row shorter than the workgroup. best and rank equal the
    restatement's, the logarithms within TOL; the rows lie between NaNs and the records between sentinels."""
    x, t = _rows(rows, V, 31 * V + rows, first_kind=V + rows)
    _check(_run_op(x, t), x, t, "V %d rows %d" % (V, rows))


@pytest.mark.parametrize("V", [1000, 51865, 52300])
def test_op_with_a_row_stride(V):
    """rowStride > nVocab: the floats between two rows are NaN and are not read."""
    x, t = _rows(6, V, V + 5)
    _check(_run_op(x, t, stride=V + 37), x, t, "V %d stride %d" % (V, V + 37))


@pytest.mark.parametrize("V", [1000, 51865])
def test_op_same_bits_in_any_place_and_from_both_forms(V):
    """A row gives the same record at row 0 of 1 and at row 64 of 65, and from the register form and the two-read form (option score_regs)."""
    x, t = _rows(65, V, 977 + V)
    assert V <= SC_REG_MAX
    all65 = _run_op(x, t)
    alone = _run_op(x[64:65], t[64:65])
    assert alone.tobytes() == all65[64:65].tobytes()
    with options(score_regs=0):
        two_reads = _run_op(x, t)
        assert _run_op(x[64:65], t[64:65]).tobytes() == alone.tobytes()
    assert two_reads.tobytes() == all65.tobytes()


def test_op_refusals():
    """Before any launch: a target outside the row, rowStride < nVocab, a null pointer, rows < 1. The destination keeps its sentinel."""
    L = binding.lib()
    V = 1000
    x = dev(np.zeros((2, V), np.float32))
    out = torch.full((8,), SENTINEL, dtype=torch.int32, device="cuda")
    ok, neg, big = dev(np.array([0, V - 1], np.int32)), dev(np.array([0, -1], np.int32)), dev(np.array([V, 0], np.int32))
    assert L.wh_op_token_scores(None, ptr(x), V, 2, V, ptr(neg), ptr(out)) == -1 and b"outside" in L.wh_last_error()
    assert L.wh_op_token_scores(None, ptr(x), V, 2, V, ptr(big), ptr(out)) == -1
    assert L.wh_op_token_scores(None, ptr(x), V - 1, 2, V, ptr(ok), ptr(out)) == -1
    assert L.wh_op_token_scores(None, ptr(x), V, 0, V, ptr(ok), ptr(out)) == -1
    assert L.wh_op_token_scores(None, None, V, 2, V, ptr(ok), ptr(out)) == -1
    assert L.wh_op_token_scores(None, ptr(x), V, 2, V, None, ptr(out)) == -1
    assert L.wh_op_token_scores(None, ptr(x), V, 2, V, ptr(ok), None) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    assert L.wh_op_token_scores(None, ptr(x), V, 2, V, ptr(ok), ptr(out)) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(REC)
    assert np.array_equal(got["best"], [0, 0]) and np.array_equal(got["rank"], [0, V - 1])


# ---------------------------------------------------------------------------------------------------------------------
# 2. wh_score_tokens against the oracles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "ref_score_d128.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def scored(gold):
    """The model and the three windows of the fixture on the device, and the records of one call over all of them (computed once, never changed)."""
    assert (gold["model_seed"], gold["mel_seed"]) == (mk.MODEL_SEED, mk.MEL_SEED)
    model = binding.HipModel.from_ggml(mk.model())
    mels = torch.from_numpy(mk.mels()).cuda()
    ctx = binding.HipContext(model, len(mk.LENS))
    ctx.encode(mels)
    rows = [w["row"] for w in gold["windows"]]
    recs = ctx.score_tokens(rows, [len(r) for r in rows], [w["first"] for w in gold["windows"]])
    recs.setflags(write=False)
    yield dict(model=model, mels=mels, ctx=ctx, rows=rows, recs=recs)
    ctx.close()
    model.close()


def _against_truth(gold, windows, recs, note):
    """The standing criterion on the log-probabilities, best and rank against WhisperTruth's; returns the largest distance."""
    dist, exceptions, n = [], 0, 0
    # an order of two ids may flip only where truth holds them closer than twice the largest deviation of a logit; the deviation allowed is the criterion's own
    flip = 2.0 * 1.25 * gold["np_logit_dev_max"]
    for b, w in windows:
        for e in w["entries"]:
            r = recs[b][e["i"]]
            n += 1
            dist.append(abs(float(r["logprob"]) - e["logprob"]))
            assert abs(float(r["bestLogprob"]) - e["bestLogprob"]) <= 1.25 * gold["np_logprob_dist_max"] + 1e-6, (note, b, e["i"])
            if int(r["best"]) != e["best"]:
                assert e["top2_margin"] < flip, (note, b, e["i"], "best", int(r["best"]), e["best"])
                exceptions += 1
            elif int(r["rank"]) != e["rank"]:
                assert e["target_margin"] < flip, (note, b, e["i"], "rank", int(r["rank"]), e["rank"])
                exceptions += 1
    dist = np.array(dist)
    print("%s: |logprob - truth| max %.3e mean %.3e over %d entries (WhisperNP: max %.3e mean %.3e), %d order exceptions" %
          (note, dist.max(), dist.mean(), n, gold["np_logprob_dist_max"], gold["np_logprob_dist_mean"], exceptions))
    assert dist.max() <= 1.25 * gold["np_logprob_dist_max"] and dist.mean() <= 1.25 * gold["np_logprob_dist_mean"], (note, dist.max(), dist.mean())
    assert exceptions <= 0.02 * n
    return float(dist.max())


def test_score_tokens_against_the_oracles(gold, scored):
    """Three windows of different audio, rows of 5, 12 and 40 tokens (54 scored rows of 57: the product crosses 32 rows, the rows are ragged), firstScored
    4, 6 and 5. Model seed 10, audio seed 17. For every scored entry: best and rank are WhisperTruth's (an exception only where truth's margin between the two ids
    concerned is below twice the largest logit deviation the criterion allows, 2 x 1.25 x 3.64e-3, and for at most 2 % of the entries -- the restatement itself
    needs none), and |logprob - truth| <= 1.25 x |WhisperNP - truth| for the largest and the mean distance: WhisperNP's own distances, computed on the CPU by
    tests/golden/make_golden_score.py, are 7.71e-4 and 2.48e-4. Entries that are not scored are zero."""
    recs = scored["recs"]
    assert gold["np_rank_or_best_differs"] == 0
    _against_truth(gold, list(enumerate(gold["windows"])), recs, "3 windows")
    keep = np.zeros(recs.shape, bool)
    for b, w in enumerate(gold["windows"]):
        keep[b, w["first"]:len(w["row"])] = True
        assert recs["rank"][b, w["first"]:len(w["row"])].max() == 0 and (recs["logprob"][b, w["first"]:len(w["row"])] < 0).all()
    assert not np.frombuffer(recs[~keep].tobytes(), np.uint8).any(), "an entry that is not scored is not zero"


def test_score_tokens_same_bits_whatever_the_chunk(scored):
    """score_chunk_rows = 8: every chunk boundary falls inside a window, and the records are the unchunked ones bit for bit."""
    rows = scored["rows"]
    firsts = [4, 6, 5]
    with options(score_chunk_rows=8):
        got = scored["ctx"].score_tokens(rows, [len(r) for r in rows], firsts)
    assert got.tobytes() == scored["recs"].tobytes()
    with options(score_chunk_rows=1, score_regs=0):
        got = scored["ctx"].score_tokens(rows, [len(r) for r in rows], firsts)
    assert got.tobytes() == scored["recs"].tobytes()


def test_score_tokens_alone_and_in_a_batch(gold, scored):
    """Window 2 scored alone (a context of one window) against the same window as the third of three: the pass picks its product kernels by the total number
    of rows, so the two are not bit for bit; each meets the criterion against truth, and they agree in best and rank."""
    ctx1 = binding.HipContext(scored["model"], 1)
    ctx1.encode(scored["mels"][2:3].contiguous())
    w = gold["windows"][2]
    alone = ctx1.score_tokens([w["row"]], [len(w["row"])], [w["first"]])
    ctx1.close()
    _against_truth(gold, [(0, w)], alone, "window 2 alone")
    sl = slice(w["first"], len(w["row"]))
    assert np.array_equal(alone["best"][0, sl], scored["recs"]["best"][2, sl]) and np.array_equal(alone["rank"][0, sl], scored["recs"]["rank"][2, sl])
    d = np.abs(alone["logprob"][0, sl].astype(np.float64) - scored["recs"]["logprob"][2, sl])
    print("alone against third of three: largest |difference| %.3e" % d.max())
    assert d.max() <= 2.0 * 1.25 * gold["np_logprob_dist_max"]


def test_a_corrupted_transcript_scores_lower(gold, scored):
    """The greedy transcript of window 2 against the same row with every third text token replaced: the sum of the log-probabilities falls by at least ten
    times the largest distance the criterion allows per entry, summed over the row (truth: the margin recorded by the fixture)."""
    w = gold["windows"][2]
    bad = scored["ctx"].score_tokens(scored["rows"][:2] + [w["bad"]], [5, 12, 40], [4, 6, 5])
    sl = slice(w["first"], len(w["row"]))
    good_sum, bad_sum = float(scored["recs"]["logprob"][2, sl].astype(np.float64).sum()), float(bad["logprob"][2, sl].astype(np.float64).sum())
    truth_good, truth_bad = sum(e["logprob"] for e in w["entries"]), sum(e["logprob"] for e in w["bad_entries"])
    n = len(w["entries"])
    per_row = 1.25 * gold["np_logprob_dist_max"]
    print("sum of log-probabilities: %.3f, corrupted %.3f (truth %.3f and %.3f)" % (good_sum, bad_sum, truth_good, truth_bad))
    assert truth_good - truth_bad >= 10 * n * per_row
    assert good_sum - bad_sum >= 10 * n * per_row
    # (a replaced token is an unlikely one: its log-probability moves with its own logit, by at most the logit deviation the criterion allows, twice)
    assert abs(good_sum - truth_good) <= n * per_row and abs(bad_sum - truth_bad) <= n * 2.0 * 1.25 * gold["np_logit_dev_max"]
    # the first two windows are what they were: a window's records do not depend on its neighbours' tokens
    assert bad[:2].tobytes() == scored["recs"][:2].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 3. nothing else moves; the refusals
# ---------------------------------------------------------------------------------------------------------------------
def _decoded(ctx, mels, sp_prompt):
    """A fresh encode, a greedy window of the device-side loop and a host-stepped wh_decode: everything a later run reads"""
    ctx.encode(mels)
    ctx.decode_window_start(sp_prompt, 12)
    data = ctx.decode_window_fetch_data(0, 13)
    ctx.decode_window_finish()
    logits, probs = ctx.decode(sp_prompt, 0)
    return data, logits, probs


def test_a_context_that_scored_decodes_as_one_that_never_did(gold, scored):
    """Greedy transcript and wh_decode of a context before wh_score_tokens, and after it behind a new wh_encode: bit-identical to those of a context that never
    scored. The feature's buffers appear with the first call only."""
    model, mels = scored["model"], scored["mels"]
    prompt = np.array([w["row"][:4] for w in gold["windows"]], np.int32)
    a, b = binding.HipContext(model, 3), binding.HipContext(model, 3)
    before = _decoded(a, mels, prompt)
    never = _decoded(b, mels, prompt)
    vram = a.vram_bytes()
    assert vram == b.vram_bytes()
    rows = scored["rows"]
    recs = a.score_tokens(rows, [len(r) for r in rows], [4, 6, 5])
    assert recs.tobytes() == scored["recs"].tobytes()
    assert a.vram_bytes() > vram and b.vram_bytes() == vram
    after = _decoded(a, mels, prompt)
    for got in (before, after):
        for k in never[0]:
            assert np.array_equal(np.ascontiguousarray(got[0][k]).view(np.uint32), np.ascontiguousarray(never[0][k]).view(np.uint32)), k
        assert np.array_equal(got[1].view(np.uint32), never[1].view(np.uint32)) and np.array_equal(got[2].view(np.uint32), never[2].view(np.uint32))
    a.close()
    b.close()


def test_score_tokens_refusals(gold, scored):
    model, mels, rows = scored["model"], scored["mels"], scored["rows"]
    lens, firsts = [len(r) for r in rows], [4, 6, 5]
    fresh = binding.HipContext(model, 3)
    with pytest.raises(binding.WhisperHipError, match="rc=-4"):                  # not encoded
        fresh.score_tokens(rows, lens, firsts)
    fresh.encode(mels[:2].contiguous())
    with pytest.raises(binding.WhisperHipError, match="more windows"):
        fresh.score_tokens(rows, lens, firsts)
    fresh.encode(mels)
    for bad_lens, bad_firsts, what in (([5, 12, 41], firsts, "length"), ([1, 12, 40], [1, 6, 5], "length"), (lens, [0, 6, 5], "first scored"),
                                       (lens, [5, 6, 5], "first scored"), (lens, [4, 12, 5], "first scored")):
        with pytest.raises(binding.WhisperHipError, match=what):
            fresh.score_tokens(rows, bad_lens, bad_firsts, n_max=40)
    with pytest.raises(binding.WhisperHipError, match="rc=-6"):                  # more tokens per window than the pass takes
        fresh.score_tokens([[1] * 257] * 3, [257] * 3, [1] * 3)
    with pytest.raises(binding.WhisperHipError, match="outside"):                # a token id outside the vocabulary
        fresh.score_tokens([rows[0][:4] + [model.hp.n_vocab]] + rows[1:], lens, firsts)
    fresh.set_flags(binding.WH_FLAG_PARITY_EXACT)
    with pytest.raises(binding.WhisperHipError, match="PARITY_EXACT"):
        fresh.score_tokens(rows, lens, firsts)
    fresh.close()
    groups = binding.HipContext(model, 3, hypotheses=5)
    groups.encode(mels)
    with pytest.raises(binding.WhisperHipError, match="greedy contexts only"):
        groups.score_tokens(rows, lens, firsts)
    groups.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the library: Context.score, BatchRunner.score, the flat C entries, forced alignment
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library(tmp_path_factory, scored):
    from whisper_amd import api, ggml_format as gf
    path = str(tmp_path_factory.mktemp("score") / "conditioned.bin")
    gf.write_model(path, mk.model())
    model = api.Model(path)
    rng = np.random.default_rng(23)
    # seven clips of 2 to 12 s and a transcript of text tokens for each, of different lengths
    clips = [(0.3 * rng.standard_normal(16000 * s)).astype(np.float32) for s in (12, 2, 5, 3, 7, 4, 9)]
    texts = [[int(t) for t in rng.integers(1000, 5000, 3 + 4 * i)] for i in range(7)]
    yield dict(api=api, model=model, clips=clips, texts=texts, hip=scored["model"])
    model.close()


def _compute_layer(hip_model, clips, rows, firsts):
    """HipContext.score_tokens on one encoder batch of these clips, each its own spectrogram at seek 0"""
    ctx = binding.HipContext(hip_model, len(clips))
    mels = [ctx.mel_spectrogram(dev(c)) for c in clips]
    ctx.encode_windows([(m, 0) for m in mels])
    recs = ctx.score_tokens(rows, [len(r) for r in rows], firsts)
    ctx.close()
    return recs


def _same(d, recs, first, n):
    got = np.array([(t["logprob"], t["best_logprob"], t["best"], t["rank"]) for t in d["tokens"]], REC)
    return len(d["tokens"]) == n and got.tobytes() == np.ascontiguousarray(recs[first:first + n]).tobytes()


def test_context_score_and_the_flat_c_entry(library):
    """Context.score -- tokens and text, with a past prompt, with timestamps -- gives the records HipContext.score_tokens gives on the same row of the same clip,
    bit for bit, eot included; sum and average are those of the records."""
    api, model = library["api"], library["model"]
    sp = model.special_tokens()
    ctx = api.Context(model)
    assert model.sot_sequence("en") == [sp["sot"], sp["sot"] + 1, sp["transcribe"], sp["not_"]]
    assert model.sot_sequence("de", translate=True, timestamps=True) == [sp["sot"], sp["sot"] + 3, sp["translate"]]
    for clip, text, kw, head in ((library["clips"][2], library["texts"][2], {}, model.sot_sequence("en")),
                                 (library["clips"][3], library["texts"][3], dict(prompt=[1500, 1501], timestamps=True), [sp["prev"], 1500, 1501] + model.sot_sequence("en", False, True))):
        d = ctx.score(clip, text, **kw)
        row = head + text + [sp["eot"]]
        want = _compute_layer(library["hip"], [clip], [row], [len(head)])
        assert _same(d, want[0], len(head), len(text) + 1)
        assert [t["id"] for t in d["tokens"]] == text + [sp["eot"]] and d["tokens"][0]["text"] == model.token_string(text[0])
        lp = np.array([t["logprob"] for t in d["tokens"]], np.float64)
        assert d["sum_logprob"] == float(lp.sum()) and abs(d["avg_logprob"] - lp.mean()) < 1e-12 and (lp < 0).all()
    # text goes through the model's tokenize
    words = " the quick brown fox"
    assert [t["id"] for t in ctx.score(library["clips"][1], words)["tokens"]][:-1] == model.tokenize(words)
    # the refusals of a request reach the caller
    for bad in (lambda: ctx.score(library["clips"][1][:15999], [400]), lambda: ctx.score(np.zeros(480001, np.float32), [400]), lambda: ctx.score(library["clips"][1], []),
                lambda: ctx.score(library["clips"][1], [51865]), lambda: ctx.score(library["clips"][1], [7] * 252), lambda: ctx.score(library["clips"][1], [sp["beg"] + 5], align=True)):
        with pytest.raises(api.WhisperError):
            bad()
    ctx.close()


def test_batch_runner_score_in_passes(library):
    """Seven requests on a runner of five slots: two passes, of five and of two, in request order. Each request receives the records of ITS clip and tokens: what
    HipContext.score_tokens gives for the same encoder batches, bit for bit. A request that fails its checks does not disturb its neighbours."""
    api, model = library["api"], library["model"]
    sp = model.special_tokens()
    head = model.sot_sequence("en")
    runner = api.BatchRunner(model, max_slots=5)
    items = list(zip(library["clips"], library["texts"]))
    hr, res, per = runner.score(items)
    assert hr == 0 and per == [0] * 7
    rows = [head + t + [sp["eot"]] for t in library["texts"]]
    for lo, hi in ((0, 5), (5, 7)):
        want = _compute_layer(library["hip"], library["clips"][lo:hi], rows[lo:hi], [len(head)] * (hi - lo))
        for i in range(lo, hi):
            assert _same(res[i], want[i - lo], len(head), len(library["texts"][i]) + 1), i
    # pieces of one buffer, and a failing request (an id outside the vocabulary) between good ones: the good ones form one pass of their own
    long_clip = np.concatenate(library["clips"][:2])
    pieces = [(long_clip, 0, len(library["clips"][0]), library["texts"][0]), (long_clip, 0, 0, [51865]), (long_clip, len(library["clips"][0]), 0, library["texts"][1])]
    hr, res2, per2 = runner.score(pieces)
    assert hr == 0x80070057 and per2 == [0, 0x80070057, 0] and res2[1] is None
    want = _compute_layer(library["hip"], library["clips"][:2], rows[:2], [len(head)] * 2)
    assert _same(res2[0], want[0], len(head), len(library["texts"][0]) + 1) and _same(res2[2], want[1], len(head), len(library["texts"][1]) + 1)
    runner.close()


def test_forced_alignment_gives_the_times_of_a_run_with_align_tokens(library):
    """A 12 s clip is one window for the conditioned model (its closing timestamp lies behind the clip's end). The text tokens runFull transcribes with
    ALIGN_TOKENS, scored with align: every text token receives the run's t0 / t1, eot the end of the text; the scores are those of the same call without align."""
    api, model = library["api"], library["model"]
    sp = model.special_tokens()
    ctx = api.Context(model)
    clip = library["clips"][0]
    assert ctx.run_full(clip, flags=api.ALIGN_TOKENS) == 0
    toks = [t for s in ctx.results() for t in s["tokens"] if t["id"] < sp["eot"]]
    assert len(toks) >= 10
    text = [t["id"] for t in toks]
    aligned = ctx.score(clip, text, align=True)
    plain = ctx.score(clip, text)
    assert [(t["t0"], t["t1"]) for t in aligned["tokens"][:-1]] == [(t["t0"], t["t1"]) for t in toks]
    assert aligned["tokens"][-1]["t0"] == aligned["tokens"][-1]["t1"] == toks[-1]["t1"]
    assert any(t["t1"] > t["t0"] for t in aligned["tokens"]) and "t0" not in plain["tokens"][0]
    strip = lambda d: [(t["id"], t["logprob"], t["best"], t["best_logprob"], t["rank"]) for t in d["tokens"]]
    assert strip(aligned) == strip(plain) and aligned["sum_logprob"] == plain["sum_logprob"]
    ctx.close()


def test_whisper_main_score(tmp_path, library):
    """whisper-main --score FILE prints one line per token of the transcript and of eot -- with --align the token's time in front --, then a summary line with the
    sum Context.score gives the same clip and text; -h does not mention the option."""
    import subprocess
    import wave
    from whisper_amd import build, ggml_format as gf
    api, model = library["api"], library["model"]
    path = str(tmp_path / "m.bin")
    gf.write_model(path, mk.model())
    clip = np.clip(np.round(library["clips"][2] * 32768.0), -32768, 32767).astype("<i2")
    wav = str(tmp_path / "a.wav")
    with wave.open(wav, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(clip.tobytes())
    words = " the quick brown fox jumps"
    txt = str(tmp_path / "a.txt")
    with open(txt, "w") as f:
        f.write(words + "\n")
    n = len(model.tokenize(words)) + 1

    def run(*args):
        r = subprocess.run([build.CLI_BIN] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        return r.returncode, r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")

    rc, out, err = run("-m", path, "-f", wav, "--score", txt)
    lines = out.strip().splitlines()
    assert rc == 0 and len(lines) == n + 1, (rc, out, err[-2000:])
    ctx = api.Context(model)
    want = ctx.score(clip.astype(np.float32) / 32768.0, words)
    ctx.close()
    assert "%d tokens" % n in lines[-1] and "sum_logprob %.4f" % want["sum_logprob"] in lines[-1]
    assert [int(ln.split()[1]) for ln in lines[:-1]] == [t["rank"] for t in want["tokens"]]
    rc, out2, err = run("--score", txt, "--align", "-m", path, "-f", wav)
    lines2 = out2.strip().splitlines()
    assert rc == 0 and len(lines2) == n + 1 and all(ln.startswith("[") and "-->" in ln for ln in lines2[:-1]) and lines2[-1] == lines[-1], (rc, out2, err[-2000:])
    h = run("-h")
    assert "--score" not in h[1] + h[2]
    assert run("--score")[0] == 2
