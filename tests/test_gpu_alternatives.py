"""GPU tests of token alternatives ("Token alternatives"): wh_op_top_logprobs against the float64 restatement (tests/alternatives_ref.py),
the device-side loop with wh_context_set_alternatives on, the library, and the refusals."""
import ctypes as C
import json
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import alternatives_ref as R  # noqa: E402
import test_gpu_timestamp_rules as T  # noqa: E402  (its helpers: windows, prompts, device buffers)
from whisper_amd import binding, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

dev, ptr, same_records = T.dev, T.ptr, T.same_records
DT = binding.TOKEN_ALTERNATIVE_DTYPE
G = 1024                                                                         # NaN guard band, floats, before and behind the rows
CONTENTS = ("normal", "max_first", "max_last", "ties", "all_equal", "neg_inf", "three_finite")


def _rows(kind, rows, V, rng):
    x = (3.0 * rng.standard_normal((rows, V))).astype(np.float32)
    for r in range(rows):
        order = rng.permutation(V)
        if kind == "max_first":
            x[r, 0] = 40.0
        elif kind == "max_last":
            x[r, V - 1] = 40.0
        elif kind == "ties":                                                     # 3 equal values on top of up to 12 equal values: the k-th place of k = 1, 5, 8 lies inside a group
            x[r, order[:min(15, V)]] = 20.0
            x[r, order[:min(3, V // 2)]] = 21.0
        elif kind == "all_equal":
            x[r] = -1.5
        elif kind == "neg_inf":                                                  # ranges as the timestamp rules leave them, and NaNs, which are never listed
            x[r, :V // 3] = -np.inf
            x[r, V // 2:V // 2 + V // 4] = -np.inf
            x[r, order[:2]] = np.nan
        elif kind == "three_finite":
            x[r, order[3:]] = -np.inf
            x[r, order[3]] = np.nan
    return x


def _launch(buf, first_float, stride, rows, V, k):
    out = torch.full((rows * k * 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    binding.op_top_logprobs(C.c_void_p(buf.data_ptr() + 4 * first_float), stride, rows, V, k, ptr(out))
    torch.cuda.synchronize()
    return np.frombuffer(out.cpu().numpy().tobytes(), DT).reshape(rows, k)


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("V,stride", [(5, 5), (8, 8), (1023, 1023), (1025, 1025), (51865, 51865), (1025, 1031)])
def test_op_against_the_float64_restatement(V, stride, rows):
    """Every kind of row at k = 1, 5, 8 (k <= V; V = 5 and 8 are rows with nVocab = k), rowStride = V so that odd rows start misaligned, and once with a gap of NaN
    between the rows; NaN guard bands around the buffer. Ids exactly; logprobs within one FP32 ulp at the reference value plus 1e-6 (a half-ulp final rounding;
    FP32 exp terms at <= 2 ulp, summed in FP64, move lse by < 5e-7); { -1, -inf } where the reference has it; the records at k = j the first j at k = 8 bit for
    bit; every row alone the bits it has among its neighbours."""
    rng = np.random.default_rng(V * 8 + rows)
    ks = [k for k in (1, 5, 8) if k <= V]
    for kind in CONTENTS:
        x = _rows(kind, rows, V, rng)
        flat = np.full(G + rows * stride + G, np.nan, np.float32)
        for r in range(rows):
            flat[G + r * stride:G + r * stride + V] = x[r]
        buf = dev(flat)
        got = {k: _launch(buf, G, stride, rows, V, k) for k in ks}
        for r in range(rows):
            want_ids, want_lp = R.top_logprobs(x[r], ks[-1])
            for k in ks:
                g, live = got[k][r], want_ids[:k] >= 0
                assert np.array_equal(g["id"], want_ids[:k]) and np.isneginf(g["logprob"][~live]).all(), (kind, r, k, g["id"], want_ids[:k])
                d = np.abs(g["logprob"][live].astype(np.float64) - want_lp[:k][live])
                assert (d <= np.spacing(np.abs(want_lp[:k][live]).astype(np.float32)).astype(np.float64) + 1e-6).all(), (kind, r, k, d.max())
                assert g.tobytes() == got[ks[-1]][r][:k].tobytes(), (kind, r, k)
            assert _launch(buf, G + r * stride, stride, 1, V, ks[-1])[0].tobytes() == got[ks[-1]][r].tobytes(), (kind, r)
        if kind == "three_finite" and V > 3:
            assert (got[ks[-1]][:, 3:]["id"] == -1).all()


@pytest.fixture(scope="module")
def net():
    hp = gf.hparams_for("test-d128-ml")
    ggml = gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=4)
    c = SimpleNamespace(hp=hp, model=binding.HipModel.from_ggml(ggml), sp=gf.special_tokens(hp))
    yield c
    c.model.close()


def _window(ctx, prompt, n_steps, chunk=0):
    """T._window with the alternatives read before the window ends: ( records, alternatives [1 + n_steps][batch][k] )"""
    ctx.decode_window_start(prompt, chunk or n_steps)
    for _ in range(n_steps // chunk - 1 if chunk else 0):
        ctx.decode_window_continue(chunk)
    data, alts = ctx.decode_window_fetch_data(0, 1 + n_steps), ctx.window_alternatives(0, 1 + n_steps)
    ctx.decode_window_finish()
    return data, alts


def _p_agrees(listed, emitted_id, p, V):
    """Where the emitted id is among the listed ( id, logprob ), exp( logprob ) against the sampler's p at the bound DESIGN.md section 7 derives from the table
    softmax's formats (the issue cites tests/test_gpu_decode_step_ops.py for it, which holds no sampler). Returns whether it was listed."""
    hit = [lp for i, lp in listed if i == emitted_id]
    if hit:
        bound = (listed[0][1] - hit[0] + 1.0) * 2.0 ** -11 + 18.4 * 2.0 ** -11 + V * 2.0 ** -25 + 1e-6
        assert abs(np.exp(hit[0]) / p - 1.0) <= bound, (emitted_id, listed, p, bound)
    return bool(hit)


@pytest.mark.parametrize("batch", [3, 5])
def test_device_loop_records_the_row_the_sampler_saw(net, batch):
    """3 windows go through the spread sampler, 5 through the one-workgroup sampler; prompt + 6 steps, k = 5. The wh_token_data are the bits of a run with the
    setting off; on / off / on again captures one graph for the setting and none after it; a start of 3 steps and a chunk behind it gives the same records. Per
    sample: distinct ids, logprobs non-increasing and <= 0, and exp( logprob ) agrees with the sample's p where the emitted id is listed. With the entry 0 of a
    step of the plain run suppressed, no listed id of any step is in the set."""
    sp, V, k, n_steps = net.sp, net.hp.n_vocab, 5, 6
    prompt = T._prompts4(sp, batch)
    ctx = binding.HipContext(net.model, batch)
    ctx.encode(T._mels(batch))
    off = T._window(ctx, prompt, n_steps)
    base = ctx.step_captures()
    ctx.set_alternatives(k)
    on, alts = _window(ctx, prompt, n_steps)
    assert same_records(on, off) and ctx.step_captures() == base + 1
    ctx.set_alternatives(0)
    assert same_records(T._window(ctx, prompt, n_steps), off)
    ctx.set_alternatives(k)
    again, alts2 = _window(ctx, prompt, n_steps, chunk=3)
    assert same_records(again, off) and alts2.tobytes() == alts.tobytes() and ctx.step_captures() == base + 1
    ids, lp = alts["id"], alts["logprob"].astype(np.float64)
    assert alts.shape == (1 + n_steps, batch, k) and ((ids >= 0) & (ids < V)).all()
    assert all(len(set(ids[s, b])) == k for s in range(1 + n_steps) for b in range(batch))
    assert (np.diff(lp, axis=2) <= 0).all() and (lp <= 0).all()
    assert sum(_p_agrees(list(zip(ids[s, b], lp[s, b])), on["id"][s, b], float(on["p"][s, b]), V) for s in range(1 + n_steps) for b in range(batch)) > 0
    banned = sorted({int(t) for t in ids[2:, :, 0].ravel() if t < sp["eot"]})
    assert banned
    ctx.set_suppress(banned)
    assert not (set(_window(ctx, prompt, n_steps)[1]["id"].ravel().tolist()) & set(banned))
    ctx.close()


@pytest.mark.parametrize("fallback", [False, True])
def test_library_keeps_the_records_of_every_result_token(tmp_path, fallback):
    """Context.set_alternatives( 3 ) on the scripted model (the multi_window case of tests/golden/ref_hostloop.json), whose rows are peaked: results() equals the
    run without it; alternatives() is parallel to it segment by segment and token by token, and entry 0 is the emitted id at every token. With the fallback
    forcing every attempt (logprob_thold = +1, as test_gpu_fallback.py does; the accepted one draws at temperature 1.0, the distribution the records describe) the
    arrays still line up with the accepted attempt's tokens: wherever the emitted id is listed, exp( logprob ) agrees with that very token's p. After
    set_alternatives( 0 ) alternatives() is empty; beam search with the setting on is E_NOTIMPL and runs once it is cleared."""
    from whisper_amd import api
    import test_batch_api as BA
    c = {c["name"]: c for c in json.load(open(BA.HOSTLOOP))["cases"]}["multi_window"]
    pcm = (0.05 * np.random.default_rng(c["pcm_seed"]).standard_normal(c["n_samples"])).astype(np.float32)
    kw = dict(flags=api.NO_CONTEXT, prompt=c["prompt"], n_max_text_ctx=c["n_max_text_ctx"])
    ggml = gf.scripted_model(c["script"], c["prompt_len"])
    gf.write_model(str(tmp_path / "scripted.bin"), ggml)
    model = api.Model(str(tmp_path / "scripted.bin"))
    ctx = model.create_context()
    if fallback:
        ctx.set_fallback(logprob_thold=1.0, no_speech_thold=2.0, seed=5)
    strip = lambda segs: [(s["t0"], s["t1"], s["text"], [(t["id"], t["p"]) for t in s["tokens"]]) for s in segs]   # noqa: E731
    assert ctx.run_full(pcm, **kw) == 0
    plain = strip(ctx.results())
    assert len(plain) >= 2 and ctx.alternatives() == []
    with pytest.raises(api.WhisperError):
        ctx.set_alternatives(9)
    ctx.set_alternatives(3)
    assert ctx.run_full(pcm, **kw) == 0
    segs, alts = ctx.results(), ctx.alternatives()
    assert strip(segs) == plain and [len(a) for a in alts] == [len(s["tokens"]) for s in segs]
    assert not fallback or all(w["attempts"] == 6 and w["temperature"] == 1.0 for w in ctx.window_stats())
    listed = 0
    for t, a in [(t, a) for s, sa in zip(segs, alts) for t, a in zip(s["tokens"], sa)]:
        assert len(a) == 3 and 0 >= a[0][1] >= a[1][1] >= a[2][1] and (fallback or a[0][0] == t["id"]), (t, a)
        listed += _p_agrees(a, t["id"], t["p"], ggml.hparams.n_vocab)
    assert listed > 0 and (fallback or listed == sum(len(a) for a in alts))
    ctx.set_fallback(None)
    with pytest.raises(api.WhisperError) as e:
        ctx.run_full(pcm, beam_width=2, **kw)
    assert e.value.hr & 0xFFFFFFFF == 0x80004001
    ctx.set_alternatives(0)
    assert ctx.run_full(pcm, beam_width=2, **kw) == 0 and ctx.alternatives() == []
    ctx.close()
    model.close()


def _refused(net, what):
    """The op with one bad argument (a dict; nothing may be launched), or a context brought to the call that must be refused"""
    if isinstance(what, dict):
        x, out = dev(np.zeros(64, np.float32)), dev(np.zeros(64, np.int32))
        a = dict(dict(x=ptr(x), stride=16, rows=2, V=16, k=3, out=ptr(out)), **what)
        rc = binding.lib().wh_op_top_logprobs(None, a["x"], a["stride"], a["rows"], a["V"], a["k"], a["out"])
        torch.cuda.synchronize()
        assert out.cpu().numpy().any() == (rc == 0)
        return binding.check(rc)
    ctx = binding.HipContext(net.model, 1, hypotheses=2 if what == "hyp" else 1)
    try:
        if what == "flag_then_setting":
            ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)
        if what == "setting_then_flag":
            ctx.set_alternatives(3)
            ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)
        if what == "window_started_off":
            ctx.encode(T._mels(1))
            ctx.decode_window_start(T._prompts4(net.sp, 1), 2)
            ctx.set_alternatives(3)
            ctx.window_alternatives(0, 1)
        ctx.set_alternatives({"k9": 9, "k-1": -1}.get(what, 3))
    finally:
        ctx.close()


@pytest.mark.parametrize("what,message", [
    ("k9", "k outside 0 .. 8"), ("k-1", "k outside 0 .. 8"), ("hyp", "hypothesis-group"), ("flag_then_setting", "WH_FLAG_PARITY_EXACT"),
    ("setting_then_flag", "wh_context_set_alternatives is on"), ("window_started_off", "started with wh_context_set_alternatives on"),
    (dict(x=None), "null"), (dict(out=None), "null"), (dict(k=0), "k outside 1 .. 8"), (dict(k=9), "k outside 1 .. 8"), (dict(V=0), "nVocab < 1"),
    (dict(rows=0), "rows < 1"), (dict(stride=15), "rowStride < nVocab"), (dict(V=53249, stride=53249), "53248")])
def test_refusals(net, what, message):
    _refused(net, {})                                                            # the arguments every bad case departs from are good
    with pytest.raises(binding.WhisperHipError, match=message):
        _refused(net, what)
