"""GPU tests of no-repeat n-grams ("No-repeat n-grams"). Everything is compared exactly -- ids, and floats by their bits; nothing here
needs a tolerance.

  * wh_op_no_repeat_ngram step by step against the numpy restatement (tests/no_repeat_ref.py), which looks at the full history and keeps no record; its limits
    (a full history, garbage records, bad arguments);
  * the device-side loop with the option on against a host-in-the-loop emulation: wh_decode's unfiltered logits, masked by the restatement, sampled by the op
    entry points -- greedy, tempered, per-row in a ragged batch, and with all four logit filters at once;
  * models whose unfiltered loop repeats an n-gram: with the option on no row does;
  * off means off, a window inherits nothing, and a change of n is a change;
  * the library: Context / BatchRunner.set_no_repeat_ngram, the fallback's attempts, the refusals, whisper-main -nrn.
The models are conditioned_model( conditioned_layout( hparams_for( "test-d128-ml" ) ), 4, ..., alpha = 30 ): at the default alpha = 10 every text position of the
layout has candidates of its own and no greedy window repeats a text token before eot, whatever the seed; with the cross-attention three times as strong the
tokens the audio favours win at several positions, or for ever -- the repetition loop of a real checkpoint. The CPU twin: tests/test_no_repeat_cpu.py."""
import ctypes as C
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import no_repeat_ref as R  # noqa: E402
import phrase_boost_ref as PB  # noqa: E402
import timestamp_rules_ref as TS  # noqa: E402
import test_gpu_timestamp_rules as T  # noqa: E402  (its helpers: windows, the samplers' op entry points, recordings)
from whisper_amd import binding, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = T.FIELDS
E_NOTIMPL, E_INVALIDARG = 0x80004001, 0x80070057
dev, ptr, same_records = T.dev, T.ptr, T.same_records
ALPHA = 30.0


# ---------------------------------------------------------------------------------------------------------------------
# 1. the op
# ---------------------------------------------------------------------------------------------------------------------
G = 4096                                                                         # guard band, elements, before and behind every buffer
FILL = 0x5A5A5A5A                                                                # what the histories hold before anything is written


class OpState:
    """logits, history and counts of one op test, each between guard bands, with the host's expectation of the two records"""

    def __init__(self, rows, V, cap, rng):
        self.rows, self.V, self.cap, self.rng = rows, V, cap, rng
        self.hist_want = np.full(G + rows * cap + G, FILL, np.int32)
        self.hist_want[:G], self.hist_want[-G:] = 0x11111111, 0x22222222
        self.cnt_want = np.full(G + rows + G, 0x33333333, np.int32)
        self.cnt_want[G:G + rows] = rng.integers(-2 ** 31, 2 ** 31 - 1, rows)    # garbage: a reset must not depend on what was there
        self.hist, self.cnt = dev(self.hist_want), dev(self.cnt_want)
        self.hist_body = C.c_void_p(self.hist.data_ptr() + 4 * G)
        self.cnt_body = C.c_void_p(self.cnt.data_ptr() + 4 * G)

    def rows_view(self):
        return self.hist_want[G:G + self.rows * self.cap].reshape(self.rows, self.cap), self.cnt_want[G:G + self.rows]

    def step(self, n, eot, fed, reset, histories, appended=None):
        """One launch on fresh random logits. histories[r]: what the restatement is asked about, None = nothing may be masked. appended[r]: the token that must
        have been written at the row's old count, None = no write to the history."""
        rows, V = self.rows, self.V
        flat = np.full(G + rows * V + G, np.nan, np.float32)
        flat.view(np.uint32)[:G] = 0x7FC00123                                    # NaNs with a payload: a rewritten guard would lose it
        flat.view(np.uint32)[-G:] = 0x7FC00321
        x = (3.0 * self.rng.standard_normal((rows, V))).astype(np.float32)
        x[0, self.rng.integers(0, V, 40)] = np.nan
        flat[G:G + rows * V] = x.ravel()
        buf = dev(flat)
        body = C.c_void_p(buf.data_ptr() + 4 * G)
        fed_dev = dev(np.asarray(fed, np.int32)) if fed is not None else None
        binding.check(binding.lib().wh_op_no_repeat_ngram(None, body, rows, V, eot, n, ptr(fed_dev) if fed is not None else None, reset, self.hist_body,
                                                          self.cnt_body, self.cap))
        torch.cuda.synchronize()
        want = flat.copy()
        w = want[G:G + rows * V].reshape(rows, V)
        n_masked = 0
        for r in range(rows):
            if histories is not None and histories[r] is not None:
                m = R.mask(histories[r], n, eot, V)
                w[r, m] = -np.inf
                n_masked += int(m.sum())
        got = buf.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, reset, histories)
        # the -inf set is exactly the mask (the input holds no -inf), the guards included in "every other float keeps its bits" above
        assert int(np.isneginf(got).sum()) == n_masked
        h, c = self.rows_view()
        for r in range(rows):
            if reset:
                c[r] = -1 if reset == 2 else 0
            elif appended is not None and appended[r] is not None:
                pos, tok, count = appended[r]
                if pos is not None:
                    h[r, pos] = tok
                c[r] = count
        assert np.array_equal(self.hist.cpu().numpy(), self.hist_want), (n, reset)
        assert np.array_equal(self.cnt.cpu().numpy(), self.cnt_want), (n, reset, self.cnt.cpu().numpy()[G:G + rows], c)
        return n_masked


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("rows", [1, 4, 5, 9])
@pytest.mark.parametrize("V", [51864, 51865, 51866])
def test_op_step_by_step_against_the_restatement(V, rows, n):
    """Every row on a generated history of 40 tokens of its own (six ids, eot and two timestamps among them, so n-grams recur constantly; row 0 is the plain
    loop a b a b), fed token by token on fresh random logits with NaNs, between NaN guard bands; history and counts between guard bands too. After every
    step: exactly the restatement's columns are -inf, every other float keeps its bits, the history holds the fed tokens and nothing else, the counts count.
    Mid-stream a reset 2 (the next fed token is not appended, the history starts empty behind it) and a reset 1 (empty at once); neither writes a logit."""
    sp = gf.special_tokens(SimpleNamespace(n_vocab=V))
    eot, beg = sp["eot"], sp["beg"]
    rng = np.random.default_rng((V * 16 + rows) * 16 + n)
    hs = R.histories(rng, rows, 40, eot, beg)
    st = OpState(rows, V, 64, rng)
    total = st.step(n, eot, None, 1, None)                                       # the prompt step: nothing is masked, whatever the records held
    for k in range(40):
        total += st.step(n, eot, [h[k] for h in hs], 0, [h[:k + 1] for h in hs], [(k, h[k], k + 1) for h in hs])
    assert total > 0
    # armed: the fed token is the caller's and is not appended; then a history from scratch
    st.step(n, eot, None, 2, None)
    st.step(n, eot, [17] * rows, 0, [[]] * rows, [(None, None, 0)] * rows)
    for k in range(12):
        total += st.step(n, eot, [h[20 + k] for h in hs], 0, [h[20:21 + k] for h in hs], [(k, h[20 + k], k + 1) for h in hs])
    st.step(n, eot, None, 1, None)
    for k in range(n + 1):
        st.step(n, eot, [h[k] for h in hs], 0, [h[:k + 1] for h in hs], [(k, h[k], k + 1) for h in hs])


def test_op_limits():
    """cap = 16, V = 1000, three rows run to the cap and eight steps past it: a full history drops the token, nothing is written behind the row's history, and
    the mask is the one of the first 16 tokens. Then records nobody wrote -- counts of 1e9 and -5, negative and huge history entries, fed ids >= V and below
    0: no fault, no write outside the rows (the guard bands), and what is masked is what the restatement gives for the clamped record. The clamps are what is
    checked here; nothing is provoked. Last, the launcher's refusals."""
    rows, V, cap, eot, n = 3, 1000, 16, 900, 2
    rng = np.random.default_rng(5)
    ids = np.array([17, 42, 899, 900, 950, 990])
    hs = [[int(t) for t in rng.choice(ids, size=24)] for _ in range(rows)]
    hs[0] = [17, 42] * 12
    st = OpState(rows, V, cap, rng)
    st.step(n, eot, None, 1, None)
    total = 0
    for k in range(24):
        kept = min(k + 1, cap)
        total += st.step(n, eot, [h[k] for h in hs], 0, [h[:kept] for h in hs], [(k if k < cap else None, h[k], kept) for h in hs])
    assert total > 0
    # garbage records: row 0 a count far above the cap and a history of wild entries, row 1 a count below -1, row 2 a fed id outside the row
    h, c = st.rows_view()
    h[0] = [-7, 2 ** 31 - 1, 42, 42, -2 ** 31, 5000, 42, 17, 1000, 999, 42, 899, -1, 42, 0, 42]
    c[0], c[1], c[2] = 10 ** 9, -5, 3
    st.hist.copy_(torch.from_numpy(st.hist_want))
    st.cnt.copy_(torch.from_numpy(st.cnt_want))
    row2 = [int(t) for t in h[2, :3]]
    masked = st.step(n, eot, [42, 17, 5000], 0, [[int(t) for t in h[0]], [], row2 + [5000]], [(None, None, cap), (None, None, 0), (3, 5000, 4)])
    assert masked >= 4                                                           # row 0: 42 is followed by 42, 17, 899 and 0 -- and by ids that are no text column
    st.step(n, eot, [-3, 2 ** 31 - 1, -2 ** 31], 0, [[int(t) for t in h[0]], [2 ** 31 - 1], row2 + [5000, -2 ** 31]],
            [(None, None, cap), (0, 2 ** 31 - 1, 1), (4, -2 ** 31, 5)])
    # bad arguments
    L = binding.lib()
    x, fed, hist, cnt = dev(np.zeros(64, np.float32)), dev(np.zeros(4, np.int32)), dev(np.zeros(64, np.int32)), dev(np.zeros(4, np.int32))

    def ok(**kw):
        a = dict(x=ptr(x), rows=1, V=16, eot=8, n=2, fed=ptr(fed), reset=0, h=ptr(hist), c=ptr(cnt), cap=4)
        a.update(kw)
        return L.wh_op_no_repeat_ngram(None, a["x"], a["rows"], a["V"], a["eot"], a["n"], a["fed"], a["reset"], a["h"], a["c"], a["cap"])

    assert ok() == 0 and ok(fed=None, reset=1) == 0 and ok(fed=None, reset=2) == 0 and ok(eot=16) == 0 and ok(eot=0) == 0 and ok(n=8) == 0 and ok(n=1) == 0
    for bad in (dict(x=None), dict(h=None), dict(c=None), dict(fed=None), dict(rows=0), dict(V=0), dict(eot=-1), dict(eot=17), dict(n=0), dict(n=9), dict(n=-1),
                dict(reset=3), dict(reset=-1), dict(cap=0)):
        assert ok(**bad) != 0, bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the device-side loop against a host-in-the-loop emulation
# ---------------------------------------------------------------------------------------------------------------------
def _looping(seed):
    hp = gf.hparams_for("test-d128-ml")
    ggml = gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=seed, alpha=ALPHA)
    return SimpleNamespace(hp=hp, ggml=ggml, model=binding.HipModel.from_ggml(ggml), sp=gf.special_tokens(hp))


@pytest.fixture(scope="module")
def looping():
    c = _looping(4)
    yield c
    c.model.close()


def _emulate(ctx, prompt, n_steps, sp, V, filters, temperature=0.0, seed=0, nonce=0):
    """T._emulate with the mask as an argument: wh_decode (unfiltered by the loop's filters, whatever the context holds) -> filters( row, history ) on the
    host -> the op entry points pick the token. Returns the records [1 + n_steps][batch]."""
    L = binding.lib()
    batch, n_prompt = prompt.shape
    probs = torch.empty((batch, V), dtype=torch.float32, device="cuda")
    history = [[] for _ in range(batch)]
    tokens, n_past, out = prompt, 0, []
    for s in range(1 + n_steps):
        logits, _ = ctx.decode(tokens, n_past, want_probs=False)
        masked = np.stack([filters(logits[b], history[b]) for b in range(batch)])
        first = int(s == 0)
        x = dev(masked)
        if temperature > 0:
            inv_t = float(np.float32(1.0) / np.float32(temperature))
            binding.check(L.wh_op_vocab_soft_max_scaled(None, ptr(x), inv_t, ptr(probs), batch, V))
            pos = dev(np.full(batch, n_prompt - 1 + s, np.int32))
            tok = T._tokens(L.wh_op_sample_draw, probs, batch, V, sp, first, first, (seed, nonce, ptr(pos)))
        else:
            binding.check(L.wh_op_vocab_soft_max(None, ptr(x), ptr(probs), batch, V))
            tok = T._tokens(L.wh_op_sample_best, probs, batch, V, sp, first, first)
        out.append(tok.copy())
        for b in range(batch):
            history[b].append(int(tok["id"][b]))
        n_past += tokens.shape[1]
        tokens = tok["id"].astype(np.int32)[:, None]
    return {k: np.stack([o[k] for o in out]) for k in FIELDS}


def _equal(got, want):
    for k in FIELDS:
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)), (k, got[k], want[k])


@pytest.mark.parametrize("temperature", [0.0, 0.8])
@pytest.mark.parametrize("batch", [1, 4, 5])
def test_device_loop_equals_the_emulation(looping, batch, temperature):
    """wh_decode_window_start plus chunks with n = 2, 20 steps, at 1, 4 and 5 rows (the single-stream decode path and the batched one), greedy and at
    temperature 0.8 through wh_context_set_sampling, one enqueue, chunks of 4 and eager steps: token for token and bit for bit in p / pt / ptsum what the
    emulation gives. No row violates the rule, and the run differs from the one with the option off."""
    c, sp, V = looping, looping.sp, looping.hp.n_vocab
    n, n_steps, seed, nonce = 2, 20, 0xDEADBEEFCAFE, 24 * 8 + 3
    prompt = T._prompts4(sp, batch)
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(T._mels(batch))
    if temperature > 0:
        ctx.set_sampling(temperature, seed, nonce)
    off = T._window(ctx, prompt, n_steps)
    ctx.set_no_repeat(n)
    runs = [T._window(ctx, prompt, n_steps), T._window(ctx, prompt, n_steps, chunk=4)]
    ctx.set_flags(binding.WH_FLAG_NO_GRAPH)
    runs.append(T._window(ctx, prompt, n_steps, chunk=4))
    ctx.set_flags(0)
    for r in runs[1:]:
        assert same_records(r, runs[0])
    want = _emulate(ctx, prompt, n_steps, sp, V, lambda row, h: R.apply(row, h, n, sp["eot"]), temperature, seed, nonce)
    print("batch %d T %.1f: off %s | on %s" % (batch, temperature, off["id"][:, 0].tolist(), runs[0]["id"][:, 0].tolist()))
    _equal(runs[0], want)
    for b in range(batch):
        assert R.violations(runs[0]["id"][:, b], n, sp["eot"]) == [], b
    assert not np.array_equal(runs[0]["id"], off["id"])
    assert same_records({k: v[:n] for k, v in runs[0].items()}, {k: v[:n] for k, v in off.items()})       # with L < n nothing is masked
    ctx.close()


def _set_four(ctx, off, sp, boost, n):
    """Turns the four filters on with a set and a phrase chosen from `off`, the records of the unfiltered run; returns the two"""
    emitted = {int(t) for t in off["id"].ravel()}
    text = sorted(t for t in emitted if t < sp["eot"])
    suppressed = text[::3]                                                       # a third of the text tokens the unfiltered run emits
    # two tokens the unfiltered run does not emit, candidates of the layout's second and third text position
    phrase = [next((t for t in range(base, base + 4) if t not in emitted), base) for base in (2000 + 64 * 2, 2000 + 64 * 3)]
    ctx.set_suppress(suppressed)
    ctx.set_timestamp_rules(True)
    ctx.set_boost([phrase], boost)
    ctx.set_no_repeat(n)
    return suppressed, phrase


@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_all_four_filters_at_once(looping, temperature):
    """A suppressed set, the timestamp rules, a boosted phrase and n = 2 on one context, 5 rows, 20 steps: the records of the emulation that applies the four
    restatements in the launch order (suppress, rules, boost, n-grams; -inf + boost stays -inf, so the order among them does not change a row). The sampled
    rows obey the timestamp rules and the n-gram rule, and no suppressed token is sampled."""
    c, sp, V = looping, looping.sp, looping.hp.n_vocab
    batch, n, n_steps, seed, nonce, boost = 5, 2, 20, 77, 5, 8.0
    prompt = T._prompts4(sp, batch)
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(T._mels(batch))
    if temperature > 0:
        ctx.set_sampling(temperature, seed, nonce)
    off = T._window(ctx, prompt, n_steps)
    suppressed, phrase = _set_four(ctx, off, sp, boost, n)
    on = T._window(ctx, prompt, n_steps)
    assert same_records(T._window(ctx, prompt, n_steps, chunk=4), on)

    def filters(row, h):
        row = np.array(row, np.float32, copy=True)
        row[suppressed] = -np.inf
        row = TS.apply(row, h, sp["eot"], sp["beg"])
        row = PB.apply(row, [phrase], h, sp["eot"], boost)
        return R.apply(row, h, n, sp["eot"])

    want = _emulate(ctx, prompt, n_steps, sp, V, filters, temperature, seed, nonce)
    _equal(on, want)
    for b in range(batch):
        assert R.violations(on["id"][:, b], n, sp["eot"]) == [] and TS.violations(on["id"][:, b], sp["eot"], sp["beg"], V) == [], b
    assert not ({int(t) for t in on["id"].ravel()} & set(suppressed)) and not np.array_equal(on["id"], off["id"])
    ctx.close()


def test_capture_inside_continue_preserves_every_filter_state(looping):
    """WARM_PRESERVE with all four filters live: the window of test_all_four_filters_at_once (greedy) started WITHOUT steps captures nothing, so the 20 steps of
    the continue capture over the window's live state. The warm-up step appends a token to every history, moves every boost state and folds a token into every
    record, and the restore must undo it. The records equal, bit for bit, those of a context that enqueued the window in one piece -- which that test holds
    against the emulation -- and differ from the unfiltered run's. Behind the first sample, a timestamp, a token folded or appended twice shows in no mask, so the
    same is asked in mid-window: the first `split` steps run eagerly under WH_FLAG_NO_GRAPH and capture nothing, the flag goes, and the continue captures over
    records and histories that hold text. Tried with a restore that skips one buffer: without the counts the window differs at split 6 (the fed token completes
    the bigram that bans the next sample), without the records at split 14 (the fed token closes a pair). A history that is not restored holds what the first
    replayed step writes again, and moving a state twice over one token of the single two-token phrase offers the same tokens: neither can show here."""
    c, sp = looping, looping.sp
    batch, n, n_steps, boost = 5, 2, 20, 8.0
    prompt = T._prompts4(sp, batch)
    whole = binding.HipContext(c.model, batch)
    whole.encode(T._mels(batch))
    off = T._window(whole, prompt, n_steps)
    _set_four(whole, off, sp, boost, n)
    want = T._window(whole, prompt, n_steps)
    whole.close()
    print("row 0: off %s | on %s" % (off["id"][:, 0].tolist(), want["id"][:, 0].tolist()))
    assert not np.array_equal(want["id"], off["id"])
    for split in (0, 6, 14):
        ctx = binding.HipContext(c.model, batch)
        ctx.encode(T._mels(batch))
        _set_four(ctx, off, sp, boost, n)
        if split:
            ctx.set_flags(binding.WH_FLAG_NO_GRAPH)
        ctx.decode_window_start(prompt, split)
        ctx.set_flags(0)
        assert ctx.step_captures() == 0
        ctx.decode_window_continue(n_steps - split)
        assert ctx.step_captures() == 1
        got = ctx.decode_window_fetch_data(0, 1 + n_steps)
        ctx.decode_window_finish()
        ctx.close()
        assert same_records(got, want), split


def test_ragged_per_row_batch_equals_the_emulation(looping):
    """6 rows, ragged prompts through wh_decode_window_start_ragged, rows 1 and 4 sampled (0.8 and 0.5) and the others greedy through
    wh_context_set_sampling_rows, n = 2, one enqueue and chunks of 4. The rows with full-length prompts (1 and 4 sampled, 3 greedy) are replayed through
    wh_decode -- the device's own tokens fed back -- the restatement's mask and the per-row op on the masked logits: their records, bit for bit, as
    tests/test_gpu_timestamp_rules.py replays its own. Every row obeys the rule."""
    c, sp, V = looping, looping.sp, looping.hp.n_vocab
    batch, n, n_steps, n_max = 6, 2, 12, 6
    lens = [3, n_max, 4, n_max, n_max, 3]
    prompts = []
    for b, ln in enumerate(lens):
        head = [sp["prev"]] + [1000 + 7 * b + i for i in range(ln - 4)] if ln > 3 else []
        prompts.append((head + [sp["sot"], sp["sot"] + 1 + b, sp["transcribe"]])[-ln:])
    assert [len(p) for p in prompts] == lens
    temps = np.array([0, 0.8, 0, 0, 0.5, 0], np.float32)
    seeds = np.array([1, 0xDEADBEEFCAFE, 2, 3, 2 ** 63 + 11, 4], np.uint64)
    nonces = np.array([0, 24 * 8 + 3, 0, 0, 7, 0], np.uint32)
    full = [1, 3, 4]

    def ragged(chunk=0):
        if chunk:
            ctx.decode_window_start_ragged(prompts, 0)
            for _ in range(n_steps // chunk):
                ctx.decode_window_continue(chunk)
        else:
            ctx.decode_window_start_ragged(prompts, n_steps)
        data = ctx.decode_window_fetch_data(0, 1 + n_steps)
        ctx.decode_window_finish()
        return data

    ctx = binding.HipContext(c.model, batch)
    ctx.encode(T._mels(batch))
    ctx.set_sampling_rows(temps, seeds, nonces)
    off = ragged()
    ctx.set_no_repeat(n)
    on = ragged()
    assert same_records(ragged(chunk=4), on)
    print("ragged: off %s | on %s" % (off["id"].T.tolist(), on["id"].T.tolist()))
    for b in range(batch):
        assert R.violations(on["id"][:, b], n, sp["eot"]) == [], b
    padded = np.zeros((batch, n_max), np.int32)
    for b, p in enumerate(prompts):
        padded[b, :len(p)] = p
    tokens, n_past = padded, 0
    for s in range(1 + n_steps):
        logits, _ = ctx.decode(tokens, n_past, want_probs=False)
        masked = np.stack([R.apply(logits[b], on["id"][:s, b], n, sp["eot"]) for b in range(batch)])
        pos = dev(np.full(batch, n_max - 1 + s, np.int32))
        first = int(s == 0)
        tok = T._sample_rows(dev(masked), batch, V, sp, first, first, temps, seeds, nonces, pos)
        for r in full:
            got = {k: on[k][s, r:r + 1] for k in FIELDS}
            assert same_records(got, tok[r:r + 1]), (s, r, {k: got[k] for k in FIELDS}, tok[r])
        n_past += tokens.shape[1]
        tokens = on["id"][s].astype(np.int32)[:, None].copy()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the test that bites
# ---------------------------------------------------------------------------------------------------------------------
def _until_eot(ids, eot):
    ids = [int(t) for t in ids]
    return ids[:ids.index(eot) + 1] if eot in ids else ids


@pytest.mark.parametrize("model_seed,n", [(4, 3), (9, 2)])
def test_a_window_that_repeats_an_ngram_repeats_none_with_the_option_on(model_seed, n):
    """How the seeds were found: on the CPU, oracle/whisper_np.py (WhisperNP.decode with exact_pv = False, sample_best with the forced initial timestamp on
    the first sample) decoded 24 steps, or up to eot, behind the prompt [prev, 1000, sot, sot + 1] on uniform( -1, 1 ) mel rows (generator seed 17), and
    tests/no_repeat_ref.violations read each sequence.
    conditioned_model( conditioned_layout, 4, "test-d128-ml", seed ) as it stands, seeds 1 .. 120: 0 of 120 repeat an n-gram that ends in a text token, for
    n = 1, 2, 3 or 4 -- every text position of the layout has four candidates of its own, so before eot no text token can come twice. The same models with
    alpha = 30 (the cross-attention output three times as strong, nothing else changed), seeds 1 .. 40: 7 of 40 repeat a 2-gram before eot (2, 4, 7, 8, 9,
    21, 37) and 3 of 40 a 3-gram (2, 4, 37). Chosen: seed 4, which samples 2066 four times in a row at samples 5 .. 8 and later 2128 for ever, never reaching
    eot (n = 3: samples 8 and 19 ..), and seed 9, which samples 2128 three times at samples 2 .. 4 and ends with eot (n = 2: sample 4).
    With the option off the device loop must repeat an n-gram before eot on some row (asserted: the oracle is not the device). With it on, greedy and at
    temperature 1.0, two windows in a row on other audio, 5 rows: no sample of any row lies in the mask its own prefix gives -- through eot and beyond it,
    where the loop keeps sampling."""
    c = _looping(model_seed)
    sp = c.sp
    batch, n_steps = 5, 24
    prompt = T._prompts4(sp, batch)
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(T._mels(batch))
    off = T._window(ctx, prompt, n_steps)
    broken = {b: R.violations(_until_eot(off["id"][:, b], sp["eot"]), n, sp["eot"]) for b in range(batch)}
    print("model seed %d, n %d, option off: violations before eot per row %s; row 0: %s" % (model_seed, n, broken, off["id"][:, 0].tolist()))
    assert any(broken.values())
    ctx.set_no_repeat(n)
    for temperature in (0.0, 1.0):
        ctx.set_sampling(temperature, 77, 5)
        for mel_seed in (17, 18):
            ctx.encode(T._mels(batch, mel_seed))
            on = T._window(ctx, prompt, n_steps, chunk=4 if mel_seed == 18 else 0)
            for b in range(batch):
                assert R.violations(on["id"][:, b], n, sp["eot"]) == [], (temperature, mel_seed, b, on["id"][:, b].tolist())
            if temperature == 0.0 and mel_seed == 17:
                assert not np.array_equal(on["id"], off["id"])
    ctx.close()
    c.model.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. off means off
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [2, 5])
def test_off_means_off_and_a_window_inherits_nothing(looping, batch):
    """On and off again: the records of a window -- tokens, ptsum and every other field, bit for bit -- are those of a context that never made the call. With
    the option on, a second window behind a first one equals that window on a context that never saw the first: no history survives the prompt step. n changed
    between windows, 2 -> 3 -> 2, gives what fresh contexts with that n give: no captured step of another n is replayed. wh_decode_greedy starts armed:
    firstTokens is not part of the history, so the call's first sample is the one a context without the option gives, and its samples obey the rule with the
    history starting there."""
    c, sp = looping, looping.sp
    n_steps = 16
    p1, p2 = T._prompts4(sp, batch), T._prompts4(sp, batch) + np.array([0, 13, 0, 0], np.int32)
    never = binding.HipContext(c.model, batch)
    never.encode(T._mels(batch))
    base = T._window(never, p1, n_steps)
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(T._mels(batch))
    assert same_records(T._window(ctx, p1, n_steps), base)
    ctx.set_no_repeat(0)                                                         # 0 on a context that never had it: nothing
    assert same_records(T._window(ctx, p1, n_steps), base)
    ctx.set_no_repeat(2)
    on1 = T._window(ctx, p1, n_steps)
    ctx.encode(T._mels(batch, 18))
    on2 = T._window(ctx, p2, n_steps)                                            # behind window 1, whose histories are full of other tokens
    ctx.set_no_repeat(3)
    on3 = T._window(ctx, p2, n_steps)
    ctx.set_no_repeat(2)
    assert same_records(T._window(ctx, p2, n_steps), on2)
    ctx.set_no_repeat(0)
    ctx.encode(T._mels(batch))
    assert same_records(T._window(ctx, p1, n_steps), base) and not same_records(on1, base)
    assert same_records(T._window(never, p1, n_steps), base)
    fresh = {}
    for n, want in ((2, on2), (3, on3)):
        fresh[n] = binding.HipContext(c.model, batch)
        fresh[n].set_no_repeat(n)
        fresh[n].encode(T._mels(batch, 18))
        assert same_records(T._window(fresh[n], p2, n_steps), want), n
    assert not same_records(on2, on3)
    # wh_decode_greedy behind a prompt fed by wh_decode, n = 1. firstTokens = the text token the unfiltered loop samples first when it is fed that very token,
    # found by a first unfiltered call: were firstTokens counted as a sample, that token would be forbidden at once.
    one = fresh[2]
    one.set_no_repeat(1)
    never.encode(T._mels(batch, 18))
    never.decode(p2, 0, want_logits=False, want_probs=False)
    probe, _ = never.decode_greedy(np.full(batch, 2128, np.int32), p2.shape[1], 12)
    first = probe[0].astype(np.int32)
    never.decode(p2, 0, want_logits=False, want_probs=False)
    ids_off, _ = never.decode_greedy(first, p2.shape[1], 12)
    one.decode(p2, 0, want_logits=False, want_probs=False)
    ids_on, _ = one.decode_greedy(first, p2.shape[1], 12)
    print("decode_greedy: first %s off %s on %s" % (first.tolist(), ids_off.T.tolist(), ids_on.T.tolist()))
    assert np.array_equal(ids_on[0], ids_off[0])
    for b in range(batch):
        assert R.violations(ids_on[:, b], 1, sp["eot"]) == []
    for x in [never, ctx] + list(fresh.values()):
        x.close()


def test_refusals(looping):
    c = looping
    hyp = binding.HipContext(c.model, 1, hypotheses=2)
    with pytest.raises(binding.WhisperHipError):
        hyp.set_no_repeat(2)                                                     # the histories would have to follow the beam's reorder
    hyp.set_no_repeat(0)
    hyp.close()
    ctx = binding.HipContext(c.model, 1)
    for n in (9, -1):
        with pytest.raises(binding.WhisperHipError):
            ctx.set_no_repeat(n)
    ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)
    with pytest.raises(binding.WhisperHipError):
        ctx.set_no_repeat(2)
    ctx.set_no_repeat(0)
    ctx.set_flags(0)
    ctx.set_no_repeat(2)
    with pytest.raises(binding.WhisperHipError):
        ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)                           # the exact mode while the option is on
    ctx.set_no_repeat(0)
    ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)
    ctx.set_flags(0)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the library
# ---------------------------------------------------------------------------------------------------------------------
_pcm, _key = T._pcm, T._key
RECORDINGS = ((40, 330, 7), (65, 440, 8), (12, 250, 9), (35, 520, 10))          # seconds, tone, seed; the third ends before the layout's last timestamp: one window


def _text_ids(segs, eot):
    return [t["id"] for s in segs for t in s["tokens"] if t["id"] < eot]


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """The looping model of the tests above (seed 4, alpha = 30) as a model file, and four recordings of one to three windows"""
    from whisper_amd import api
    hp = gf.hparams_for("test-d128-ml")
    ggml = gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=4, alpha=ALPHA)
    path = str(tmp_path_factory.mktemp("nrn") / "loop.bin")
    gf.write_model(path, ggml)
    model = api.Model(path)
    pcms = [_pcm(*r) for r in RECORDINGS]
    kw = dict(language="en", prompt=[1000], n_max_text_ctx=0, flags=api.NO_CONTEXT)
    ctx = model.create_context()
    yield SimpleNamespace(api=api, path=path, model=model, pcms=pcms, kw=kw, ctx=ctx, eot=gf.special_tokens(hp)["eot"])
    ctx.close()
    model.close()


def test_library_context(library):
    """Context.set_no_repeat_ngram( 2 ): run_full and run_streamed succeed on every recording and the transcripts differ from the unfiltered ones. n = 1 on the
    one-window recording: no text token comes twice in the transcript (a transcript holds a subset of its window's samples) -- greedy, and with set_fallback
    forcing every window through all attempts (the last at temperature 1.0; checked when the sampled run, too, is one window). Beam search with the option on is E_NOTIMPL and runs once it is cleared (0 and
    None both clear); cleared, the transcripts are those of a context that never made the call. n = 9 is E_INVALIDARG."""
    lb = library
    fresh = lb.model.create_context()
    plain = []
    for pcm in lb.pcms:
        assert fresh.run_full(pcm, **lb.kw) == 0
        plain.append(_key(fresh.results()))
    with pytest.raises(lb.api.WhisperError) as e:
        lb.ctx.set_no_repeat_ngram(9)
    assert e.value.hr == E_INVALIDARG
    lb.ctx.set_no_repeat_ngram(2)
    try:
        changed = 0
        for pcm, off in zip(lb.pcms, plain):
            assert lb.ctx.run_full(pcm, **lb.kw) == 0
            got = lb.ctx.results()
            assert len(got) >= 1
            changed += int(_key(got) != off)
            hr, _ = lb.ctx.run_streamed(pcm, **lb.kw)
            assert hr == 0 and len(lb.ctx.results()) >= 1
        print("n = 2: %d of %d transcripts differ from the unfiltered ones" % (changed, len(plain)))
        assert changed >= 1                                                      # the rule reached the transcripts
        lb.ctx.set_no_repeat_ngram(1)
        lb.ctx.set_fallback(logprob_thold=-1e30, entropy_thold=-1.0, no_speech_thold=2.0)                 # gates nothing fails: for the window count alone
        assert lb.ctx.run_full(lb.pcms[2], **lb.kw) == 0
        stats, ids = lb.ctx.window_stats(), _text_ids(lb.ctx.results(), lb.eot)
        assert len(stats) == 1 and stats[0]["attempts"] == 1                     # what the next assertion stands on: ONE window, decoded once
        print("n = 1, one window: text ids %s; unfiltered %s" % (ids, [t for s in plain[2] for t in s[3] if t < lb.eot]))
        assert len(ids) >= 1 and len(set(ids)) == len(ids)
        lb.ctx.set_fallback(temperature_inc=0.2, logprob_thold=1.0, entropy_thold=-1.0, no_speech_thold=2.0, seed=5)
        assert lb.ctx.run_full(lb.pcms[2], **lb.kw) == 0
        stats, ids = lb.ctx.window_stats(), _text_ids(lb.ctx.results(), lb.eot)
        print("n = 1, all attempts: %d window(s), text ids %s" % (len(stats), ids))
        assert len(stats) >= 1 and all(w["attempts"] == 6 and w["temperature"] == 1.0 for w in stats) and len(ids) >= 1
        if len(stats) == 1:                                                      # a sampled window may close early and leave audio for a second one
            assert len(set(ids)) == len(ids)
        lb.ctx.set_fallback(None)
        with pytest.raises(lb.api.WhisperError) as e:
            lb.ctx.run_full(lb.pcms[0], beam_width=2, **lb.kw)
        assert e.value.hr == E_NOTIMPL
        lb.ctx.set_no_repeat_ngram(0)
        assert lb.ctx.run_full(lb.pcms[0], beam_width=2, **lb.kw) == 0 and len(lb.ctx.results()) >= 1
        lb.ctx.set_no_repeat_ngram(3)
    finally:
        lb.ctx.set_fallback(None)
        lb.ctx.set_no_repeat_ngram(None)
    for pcm, off in zip(lb.pcms, plain):
        assert lb.ctx.run_full(pcm, **lb.kw) == 0 and _key(lb.ctx.results()) == off
    fresh.close()


def test_library_batch_runner(library):
    """BatchRunner.set_no_repeat_ngram( 2 ) with 3 slots and 4 streams: every stream's transcript -- times, text, ids -- equals Context.run_full of that stream
    with n = 2, whichever neighbours it has (the streams in another order, and one stream alone). n = 9 is E_INVALIDARG. Cleared: the transcripts of a runner
    that never made the call."""
    lb = library
    kw = dict(lb.kw, flags=lb.api.NO_CONTEXT | lb.api.SINGLE_SEGMENT)
    runner = lb.model.create_batch_runner(max_slots=3, groups=1)
    hr, never, per = runner.run(lb.pcms, **kw)
    assert hr == 0 and all(p == 0 for p in per)
    never = [_key(s) for s in never]
    with pytest.raises(lb.api.WhisperError) as e:
        runner.set_no_repeat_ngram(9)
    assert e.value.hr == E_INVALIDARG
    runner.set_no_repeat_ngram(2)
    hr, got, per = runner.run(lb.pcms, **kw)
    assert hr == 0 and all(p == 0 for p in per)
    lb.ctx.set_no_repeat_ngram(2)
    try:
        single = []
        for pcm in lb.pcms:
            assert lb.ctx.run_full(pcm, **kw) == 0
            single.append(_key(lb.ctx.results()))
    finally:
        lb.ctx.set_no_repeat_ngram(0)
    assert [_key(g) for g in got] == single and all(len(s) >= 1 for s in single)
    assert single != never
    order = [3, 1, 0, 2]
    hr, got, per = runner.run([lb.pcms[i] for i in order], **kw)
    assert hr == 0 and [_key(g) for g in got] == [single[i] for i in order]
    hr, got, per = runner.run(lb.pcms[1:2], **kw)
    assert hr == 0 and [_key(g) for g in got] == single[1:2]
    runner.set_no_repeat_ngram(None)
    hr, back, _ = runner.run(lb.pcms, **kw)
    assert hr == 0 and [_key(s) for s in back] == never
    runner.close()


def test_whisper_main_takes_the_option(library, tmp_path):
    """whisper-main -nrn 2 / --no-repeat-ngram 2 writes the transcript of the library run with n = 2, which is not the unfiltered one; -h does not mention it."""
    import wave
    from whisper_amd import build
    lb = library
    q = np.clip(np.round(lb.pcms[0] * 32768.0), -32768, 32767).astype("<i2")
    pcm = q.astype(np.float32) / 32768.0                                         # what the tool reads from the 16-bit file
    wav = str(tmp_path / "rec.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(q.tobytes())
    ctx = lb.model.create_context()                                              # a fresh one, like the tool's: no prompt carried over from earlier runs
    assert ctx.run_full(pcm) == 0
    plain = [s["text"] for s in ctx.results()]
    ctx.close()
    ctx = lb.model.create_context()
    ctx.set_no_repeat_ngram(2)
    assert ctx.run_full(pcm) == 0
    texts = [s["text"] for s in ctx.results()]
    ctx.close()

    def tool(*extra):
        r = subprocess.run([build.CLI_BIN, "-m", lb.path, "-f", wav, "-l", "en", "-nc"] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        return [ln.split(b"]  ", 1)[1] for ln in r.stdout.splitlines() if b"]  " in ln]

    assert tool("-nrn", "2") == texts and tool("--no-repeat-ngram", "2") == texts and len(texts) >= 1 and texts != plain
    bad = subprocess.run([build.CLI_BIN, "-m", lb.path, "-f", wav, "-l", "en", "-nc", "-nrn", "9"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert bad.returncode == 6
    usage = subprocess.run([build.CLI_BIN, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "-nrn" not in usage.stdout + usage.stderr and "no-repeat" not in usage.stdout + usage.stderr
