"""GPU tests of phrase boosting ("Phrase boosting"). Everything is compared bit for bit; nothing here needs a tolerance.

  * wh_op_boost_logits step by step against the brute-force restatement (tests/phrase_boost_ref.py), which tries every suffix of the history against every
    phrase and keeps no state;
  * the device-side loop with a set held against a host-in-the-loop emulation: wh_decode's unboosted logits, boosted by the restatement, sampled by the op
    entry points -- greedy, tempered, per-row in a ragged batch;
  * a property that needs no model: under a boost of 1e4 every sampled text token is an offered one;
  * off means off, and a window does not inherit the states of the one before;
  * the refusals.
The CPU twin: tests/test_phrase_boost_cpu.py."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import phrase_boost_ref as R  # noqa: E402
import timestamp_rules_ref as TS  # noqa: E402
from whisper_amd import binding, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

TOKEN_DT = np.dtype([("id", "<i4"), ("tid", "<i4"), ("p", "<f4"), ("pt", "<f4"), ("ptsum", "<f4")])
FIELDS = ("id", "tid", "p", "pt", "ptsum")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def same_records(a, b):
    """Every TokenData field, floats by their bits"""
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)) for k in FIELDS)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the op
# ---------------------------------------------------------------------------------------------------------------------
G = 4096                                                                         # NaN guard band, floats, before and behind the rows
BOOST = 2.5
STEPS = 10


def _op_step(body, rows, V, eot, tables, fed, reset, states):
    binding.check(binding.lib().wh_op_boost_logits(None, body, rows, V, eot, ptr(tables), tables.numel(), ptr(fed) if fed is not None else None, reset, ptr(states)))
    torch.cuda.synchronize()


def _run_op_case(V, eot, rows, name, phrases, seed):
    """One set: rows on different histories, STEPS steps behind a reset 1, then the second-reset protocol. Returns the columns boosted."""
    tables_host = binding.boost_compile(phrases, eot, V, BOOST)
    tables = dev(tables_host)
    rng = np.random.default_rng(seed)
    seqs = R.histories(phrases, eot, V, seed, count=rows, length=STEPS)
    states = torch.full((rows,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # garbage: the reset must not depend on what was there
    n_boosted = 0

    def fresh():
        flat = np.full(G + rows * V + G, np.nan, np.float32)
        flat.view(np.uint32)[:G] = 0x7FC00123                                    # NaNs with a payload: a rewritten guard would lose it
        flat.view(np.uint32)[-G:] = 0x7FC00321
        x = (3.0 * rng.standard_normal((rows, V))).astype(np.float32)
        x[rows - 1, rng.integers(0, V, 300)] = -np.inf
        x[0, rng.integers(0, V, 40)] = np.nan
        x[0, phrases[0][0]] = -np.inf                                            # an offered column that is suppressed stays suppressed
        flat[G:G + rows * V] = x.ravel()
        buf = dev(flat)
        return flat, buf, C.c_void_p(buf.data_ptr() + 4 * G)

    def check_step(histories, fed, reset=0):
        nonlocal n_boosted
        flat, buf, body = fresh()
        _op_step(body, rows, V, eot, tables, dev(np.asarray(fed, np.int32)) if fed is not None else None, reset, states)
        want = flat.copy()
        w = want[G:G + rows * V].reshape(rows, V)
        for r, h in enumerate(histories):
            cols = np.array(sorted(R.offered(phrases, R.tail(h, eot))), np.int64)
            w[r, cols] = w[r, cols] + np.float32(BOOST)
            n_boosted += len(cols)
        assert np.array_equal(buf.cpu().numpy().view(np.uint32), want.view(np.uint32)), (name, V, rows, histories)
        # the states are the host twin's: the same node numbers, so the restatement's in the sense tests/test_phrase_boost_cpu.py shows
        return states.cpu().numpy()

    check_step([[]] * rows, None, reset=1)                                       # the prompt step: the root's offers, whatever the states held
    twin = [0] * rows
    for k in range(STEPS):
        got = check_step([s[:k + 1] for s in seqs], [s[k] for s in seqs])
        twin = [binding.boost_step_host(tables_host, twin[r], seqs[r][k], 0, np.zeros(V, np.float32), eot)[0] for r in range(rows)]
        assert got.tolist() == twin, (name, k)
    # a second reset forgets: armed, the fed token is no sample and the history stays empty; then a history from scratch
    first = [p[0] for p in (phrases * rows)[:rows]]
    assert (check_step([[]] * rows, None, reset=2) == -1).all()
    assert (check_step([[]] * rows, [phrases[0][0]] * rows) == 0).all()
    check_step([[t] for t in first], first)
    assert (check_step([[]] * rows, None, reset=1) == 0).all()
    check_step([[t] for t in first], first)
    return n_boosted


@pytest.mark.parametrize("rows", [1, 5, 6])
@pytest.mark.parametrize("V", [51864, 51865, 51866])
def test_op_step_by_step_against_the_restatement(V, rows):
    """Every set of tests/phrase_boost_ref.sets, fed token by token, row r on another history than its neighbours; fresh random logits with NaNs, -inf and NaN
    guard bands in every step. After every step exactly the restatement's columns hold x + boost, bit for bit, every other float -- the guards included --
    keeps its bits, and the states are the host twin's. 51864 is the synthetic .en layout, 51865 the multilingual one, 51866 large-v3's: eot and the row
    starts are no multiples of 4, 32 or 64. Resets 1 and 2 boost the root's offers and fold nothing; a second reset forgets. The set "edge ids" runs a
    second time with eot == V, so that ids in the last partial 32-bit word of the row are offered."""
    sp = gf.special_tokens(SimpleNamespace(n_vocab=V))
    eot = sp["eot"]
    total = 0
    for i, (name, phrases) in enumerate(sorted(R.sets(eot).items())):
        total += _run_op_case(V, eot, rows, name, phrases, V * 64 + rows * 16 + i)
    total += _run_op_case(V, V, rows, "edge ids, eot == V", R.sets(V)["edge ids"], V + rows)
    assert total > 0


def test_op_bad_arguments():
    L = binding.lib()
    x, i, st = dev(np.zeros(16, np.float32)), dev(np.zeros(8, np.int32)), dev(np.zeros(1, np.int32))
    ok = (ptr(x), 1, 16, 8, ptr(i), 8, ptr(i), 0, ptr(st))
    for k, bad in ((0, None), (1, 0), (2, 0), (2, 65537), (3, 17), (3, -1), (4, None), (5, 3), (6, None), (7, 3), (7, -1), (8, None)):
        args = list(ok)
        args[k] = bad
        assert L.wh_op_boost_logits(None, *args) != 0, (k, bad)
    args = list(ok)
    args[6], args[7] = None, 1
    assert L.wh_op_boost_logits(None, *args) == 0                                # a reset needs no fed tokens; all-zero tables offer nothing
    torch.cuda.synchronize()
    assert (x.cpu().numpy() == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the device-side loop against a host-in-the-loop emulation
# ---------------------------------------------------------------------------------------------------------------------
LOOP_BOOST = 8.0


def _conditioned(seed):
    hp = gf.hparams_for("test-d128-ml")
    ggml = gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=seed)
    return SimpleNamespace(hp=hp, ggml=ggml, model=binding.HipModel.from_ggml(ggml), sp=gf.special_tokens(hp))


@pytest.fixture(scope="module")
def conditioned():
    c = _conditioned(10)
    yield c
    c.model.close()


def _mels(batch, seed=17):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.uniform(-1, 1, (batch, 80, 3000)).astype(np.float32)).cuda()


def _prompts4(sp, batch):
    """The prompt length the conditioned models are built for"""
    return np.array([[sp["prev"], 1000 + b, sp["sot"], sp["sot"] + 1] for b in range(batch)], np.int32)


def _window(ctx, prompt, n_steps, chunk=0):
    """prompt step + n_steps steps, in one enqueue or as a start of `chunk` steps and chunks behind it: dict of [1 + n_steps][batch] arrays"""
    if chunk:
        ctx.decode_window_start(prompt, chunk)
        for _ in range(n_steps // chunk - 1):
            ctx.decode_window_continue(chunk)
    else:
        ctx.decode_window_start(prompt, n_steps)
    data = ctx.decode_window_fetch_data(0, 1 + n_steps)
    ctx.decode_window_finish()
    return data


def _phrases_not_emitted(off_ids, shift=0):
    """Phrases over the conditioned model's text candidates (token i of a window behind a prompt of four is one of 2000 + 64 i + 0 .. 3; `shift` moves i for
    longer prompts) that the unboosted run did not emit on any row -- a foreign token where a position's four were all emitted. The second phrase begins
    inside the first: a failure link that is not the root's. The one-token phrases are offered in every step."""
    emitted = {int(t) for t in np.asarray(off_ids).ravel()}

    def pick(i, k=0):
        i += shift
        free = [2000 + 64 * i + j for j in range(4) if 2000 + 64 * i + j not in emitted] + [30000 + 7 * i, 30001 + 7 * i]
        return free[k]
    phrases = [[pick(1), pick(2), pick(3)], [pick(2), pick(3), pick(4), pick(5)], [pick(9), pick(10)], [pick(9), pick(11), pick(12)]]
    phrases += [[pick(i, 1)] for i in (1, 2, 3, 4, 8, 9, 10, 11)]
    assert not emitted & {t for p in phrases for t in p}
    return phrases


def _tokens(fn, probs_dev, rows, V, sp, force, initial, extra=()):
    out = torch.zeros(rows * 5, dtype=torch.int32, device="cuda")
    binding.check(fn(None, ptr(probs_dev), rows, V, sp["beg"], sp["sot"], sp["solm"], sp["not_"], int(force), int(initial), *extra, ptr(out)))
    torch.cuda.synchronize()
    return np.frombuffer(out.cpu().numpy().tobytes(), TOKEN_DT)


def _emulate(ctx, prompt, n_steps, sp, V, phrases, temperature=0.0, seed=0, nonce=0, rules=False):
    """wh_decode (unboosted, whatever set the context holds) -> the restatement on the host (behind the timestamp rules' restatement with `rules`: the launch
    order) -> the op entry points pick the token. Returns the records [1 + n_steps][batch]."""
    L = binding.lib()
    batch, n_prompt = prompt.shape
    probs = torch.empty((batch, V), dtype=torch.float32, device="cuda")
    history = [[] for _ in range(batch)]
    tokens, n_past, out = prompt, 0, []
    for s in range(1 + n_steps):
        logits, _ = ctx.decode(tokens, n_past, want_probs=False)
        if rules:
            logits = np.stack([TS.apply(logits[b], history[b], sp["eot"], sp["beg"]) for b in range(batch)])
        boosted = np.stack([R.apply(logits[b], phrases, history[b], sp["eot"], LOOP_BOOST) for b in range(batch)])
        first = int(s == 0)
        x = dev(boosted)
        if temperature > 0:
            inv_t = float(np.float32(1.0) / np.float32(temperature))
            binding.check(L.wh_op_vocab_soft_max_scaled(None, ptr(x), inv_t, ptr(probs), batch, V))
            pos = dev(np.full(batch, n_prompt - 1 + s, np.int32))
            tok = _tokens(L.wh_op_sample_draw, probs, batch, V, sp, first, first, (seed, nonce, ptr(pos)))
        else:
            binding.check(L.wh_op_vocab_soft_max(None, ptr(x), ptr(probs), batch, V))
            tok = _tokens(L.wh_op_sample_best, probs, batch, V, sp, first, first)
        out.append(tok.copy())
        for b in range(batch):
            history[b].append(int(tok["id"][b]))
        n_past += tokens.shape[1]
        tokens = tok["id"].astype(np.int32)[:, None]
    return {k: np.stack([o[k] for o in out]) for k in FIELDS}


@pytest.mark.parametrize("temperature", [0.0, 0.8])
@pytest.mark.parametrize("batch", [1, 4, 5])
def test_device_loop_equals_the_emulation(conditioned, batch, temperature):
    """wh_decode_window_start plus chunks with a set held, 20 steps, at 1, 4 and 5 rows (the single-stream decode path and the batched one), greedy and at
    temperature 0.8 through wh_context_set_sampling, graph replay and eager steps: token for token and bit for bit in p / pt / ptsum what the emulation gives.
    The phrases are made of tokens the unboosted run does not emit, and the boosted run differs from it."""
    c, sp, V = conditioned, conditioned.sp, conditioned.hp.n_vocab
    n_steps, seed, nonce = 20, 0xDEADBEEFCAFE, 24 * 8 + 3
    prompt = _prompts4(sp, batch)
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(_mels(batch))
    if temperature > 0:
        ctx.set_sampling(temperature, seed, nonce)
    off = _window(ctx, prompt, n_steps)
    phrases = _phrases_not_emitted(off["id"])
    ctx.set_boost(phrases, LOOP_BOOST)
    runs = [_window(ctx, prompt, n_steps), _window(ctx, prompt, n_steps, chunk=4)]
    ctx.set_flags(binding.WH_FLAG_NO_GRAPH)
    runs.append(_window(ctx, prompt, n_steps, chunk=4))
    ctx.set_flags(0)
    for r in runs[1:]:
        assert same_records(r, runs[0])
    want = _emulate(ctx, prompt, n_steps, sp, V, phrases, temperature, seed, nonce)
    print("batch %d T %.1f: off %s | on %s" % (batch, temperature, off["id"][:, 0].tolist(), runs[0]["id"][:, 0].tolist()))
    for k in FIELDS:
        assert np.array_equal(np.ascontiguousarray(runs[0][k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)), (k, runs[0][k], want[k])
    assert not np.array_equal(runs[0]["id"], off["id"])
    assert {int(t) for t in runs[0]["id"].ravel()} & {t for p in phrases for t in p}                  # a boosted token was emitted
    ctx.close()


def _sample_rows(logits_dev, rows, V, sp, force, initial, temps, seeds, nonces, pos_dev):
    L = binding.lib()
    params = (binding.SampleRowC * rows)(*[binding.SampleRowC(float(t), int(n), int(s)) for t, s, n in zip(temps, seeds, nonces)])
    probs = torch.full((rows, V), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.zeros(rows * 5, dtype=torch.int32, device="cuda")
    binding.check(L.wh_op_sample_rows(None, ptr(logits_dev), rows, V, sp["beg"], sp["sot"], sp["solm"], sp["not_"], int(force), int(initial),
                                      C.cast(params, C.c_void_p), ptr(pos_dev), ptr(probs), ptr(out)))
    torch.cuda.synchronize()
    return np.frombuffer(out.cpu().numpy().tobytes(), TOKEN_DT)


def test_ragged_per_row_batch_equals_the_emulation(conditioned):
    """6 rows, ragged prompts through wh_decode_window_start_ragged, rows 1 and 4 sampled (0.8 and 0.5) and the others greedy through
    wh_context_set_sampling_rows, a set held, one enqueue and chunks of 4. The rows with full-length prompts (1 and 4 sampled, 3 greedy) are replayed through
    wh_decode -- the device's own tokens fed back -- the restatement and the per-row op on the boosted logits: their records, bit for bit."""
    c, sp, V = conditioned, conditioned.sp, conditioned.hp.n_vocab
    batch, n_steps, n_max = 6, 12, 6
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
    ctx.encode(_mels(batch))
    ctx.set_sampling_rows(temps, seeds, nonces)
    off = ragged()
    # the model is built for a prompt of four: behind six, token i of the window sits where the layout has token i + 2
    phrases = _phrases_not_emitted(off["id"], shift=2) + _phrases_not_emitted(off["id"])
    ctx.set_boost(phrases, LOOP_BOOST)
    on = ragged()
    assert same_records(ragged(chunk=4), on) and not np.array_equal(on["id"], off["id"])
    padded = np.zeros((batch, n_max), np.int32)
    for b, p in enumerate(prompts):
        padded[b, :len(p)] = p
    tokens, n_past = padded, 0
    for s in range(1 + n_steps):
        logits, _ = ctx.decode(tokens, n_past, want_probs=False)
        boosted = np.stack([R.apply(logits[b], phrases, on["id"][:s, b], sp["eot"], LOOP_BOOST) for b in range(batch)])
        pos = dev(np.full(batch, n_max - 1 + s, np.int32))
        first = int(s == 0)
        tok = _sample_rows(dev(boosted), batch, V, sp, first, first, temps, seeds, nonces, pos)
        for r in full:
            got = {k: on[k][s, r:r + 1] for k in FIELDS}
            assert same_records(got, tok[r:r + 1]), (s, r, {k: got[k] for k in FIELDS}, tok[r])
        n_past += tokens.shape[1]
        tokens = on["id"][s].astype(np.int32)[:, None].copy()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. a property no model can break
# ---------------------------------------------------------------------------------------------------------------------
def test_under_a_huge_boost_every_text_token_is_an_offered_one(conditioned):
    """With a boost of 1e4 the offered tokens hold all the mass of a row: every sampled text token lies in O(h) of its own history, greedy and at temperature
    1.0; no timestamp but the forced first one and no eot is sampled before the token bound. With the timestamp rules and a suppressed set on as well -- the
    set holds offered tokens -- no suppressed id appears (-inf + boost is -inf) and the property still holds. No timestamp follows the forced one here, so their
    order is not at stake: test_a_moderate_boost_under_the_timestamp_rules is where boost and rules meet on rows that go on sampling timestamps."""
    c, sp, V = conditioned, conditioned.sp, conditioned.hp.n_vocab
    eot, batch, n_steps = sp["eot"], 5, 24
    phrases = [[3000, 3001, 3002], [3001, 3002, 3003, 3004], [3002, 3000], [3004], [3005, 3005, 3005], [3006, 3007], [3008]]
    prompt = _prompts4(sp, batch)
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(_mels(batch))
    ctx.set_boost(phrases, 1e4)
    for suppressed in ([], [3001, 3004, 3008]):
        ctx.set_suppress(suppressed)
        ctx.set_timestamp_rules(bool(suppressed))
        for temperature in (0.0, 1.0):
            ctx.set_sampling(temperature, 77, 5)
            ids = _window(ctx, prompt, n_steps, chunk=4 if temperature else 0)["id"]
            for b in range(batch):
                row = [int(t) for t in ids[:, b]]
                assert row[0] >= sp["beg"] and all(t < eot for t in row[1:]), (suppressed, temperature, row)
                assert not set(row) & set(suppressed)
                for k in range(1, len(row)):
                    assert row[k] in R.offered(phrases, R.tail(row[:k], eot)), (suppressed, temperature, k, row)
    ctx.close()


@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_a_moderate_boost_under_the_timestamp_rules(temperature):
    """The boost and the timestamp rules on one row, at a boost that leaves the timestamps in play: the conditioned model of seed 114, whose unfiltered window
    goes back in time (tests/test_gpu_timestamp_rules.py), 5 rows, 24 steps, the rules on and a set of phrases the plain run does not emit. The window equals
    the emulation -- the rules' restatement, then the boost's, then the op samplers -- bit for bit; it holds a boosted token; every row samples timestamps
    behind the forced first one and breaks no clause: none out of order, none unpaired."""
    c = _conditioned(114)
    sp, V = c.sp, c.hp.n_vocab
    batch, n_steps, seed, nonce = 5, 24, 77, 5
    prompt = _prompts4(sp, batch)
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(_mels(batch))
    if temperature > 0:
        ctx.set_sampling(temperature, seed, nonce)
    ctx.set_timestamp_rules(True)
    rules_only = _window(ctx, prompt, n_steps)
    phrases = _phrases_not_emitted(rules_only["id"])
    ctx.set_boost(phrases, LOOP_BOOST)
    on = _window(ctx, prompt, n_steps, chunk=4)
    want = _emulate(ctx, prompt, n_steps, sp, V, phrases, temperature, seed, nonce, rules=True)
    for k in FIELDS:
        assert np.array_equal(np.ascontiguousarray(on[k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)), (k, on[k], want[k])
    assert not np.array_equal(on["id"], rules_only["id"]) and {int(t) for t in on["id"].ravel()} & {t for p in phrases for t in p}
    for b in range(batch):
        row = [int(t) for t in on["id"][:, b]]
        assert TS.violations(row, sp["eot"], sp["beg"], V) == [], (b, row)
        stamps = [t for t in row if t >= sp["beg"]]
        assert len(stamps) >= 3 and stamps == sorted(stamps), (b, row)
    ctx.close()
    c.model.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. off means off
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [2, 5])
def test_off_means_off_and_a_window_inherits_nothing(conditioned, batch):
    """Set and cleared: the records of a window -- tokens, ptsum and every other field, bit for bit -- are those of a context that never made the call, and no
    graph was captured that such a context does not capture. With a set held, a second window behind a first one equals that window on a context that never
    saw the first: no state survives the prompt step. wh_decode_greedy counts from its own first sample: firstTokens, the head of a phrase, is not taken for
    a sampled one."""
    c, sp, V = conditioned, conditioned.sp, conditioned.hp.n_vocab
    n_steps = 16
    p1, p2 = _prompts4(sp, batch), _prompts4(sp, batch) + np.array([0, 13, 0, 0], np.int32)
    never = binding.HipContext(c.model, batch)
    never.encode(_mels(batch))
    base = _window(never, p1, n_steps)
    phrases = _phrases_not_emitted(base["id"])
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(_mels(batch))
    ctx.set_boost(phrases, LOOP_BOOST)
    ctx.set_boost(None)
    assert same_records(_window(ctx, p1, n_steps), base) and ctx.step_captures() == never.step_captures() == 1
    ctx.set_boost(phrases, LOOP_BOOST)
    on1 = _window(ctx, p1, n_steps)
    ctx.encode(_mels(batch, 18))
    on2 = _window(ctx, p2, n_steps)                                              # behind window 1, whose states end elsewhere
    assert ctx.step_captures() == 2                                              # one graph for the set, whatever the window
    ctx.set_boost([[5]], 3.0)
    ctx.set_boost(phrases, LOOP_BOOST)
    ctx.encode(_mels(batch))
    assert same_records(_window(ctx, p1, n_steps), on1) and ctx.step_captures() == 2      # another set and boost: the same graph
    ctx.set_boost([])
    assert same_records(_window(ctx, p1, n_steps), base) and not same_records(on1, base)
    assert same_records(_window(never, p1, n_steps), base)
    fresh = binding.HipContext(c.model, batch)
    fresh.set_boost(phrases, LOOP_BOOST)
    fresh.encode(_mels(batch, 18))
    assert same_records(_window(fresh, p2, n_steps), on2)
    # wh_decode_greedy behind a prompt fed by wh_decode, firstTokens = a, under the set { [a, x] }, a boost of 1e4 and a suppressed: were a counted as a
    # sample, x alone would carry the boost and be the first sample. It is not counted: the root offers a, -inf stays -inf, and the call samples what a
    # context without a set does
    a, x = 3000, 3001
    first = np.full(batch, a, np.int32)
    for z in (fresh, never):
        z.set_suppress([a])
        z.encode(_mels(batch, 18))
        z.decode(p2, 0, want_logits=False, want_probs=False)
    fresh.set_boost([[a, x]], 1e4)
    ids_on, _ = fresh.decode_greedy(first, p2.shape[1], 6)
    ids_off, _ = never.decode_greedy(first, p2.shape[1], 6)
    assert np.array_equal(ids_on, ids_off) and not (ids_on == x).any()
    # ... and from its own first sample on the history counts: the call equals the emulation, whose history starts empty at that sample
    for z in (fresh, never):
        z.set_suppress(None)
    phrases = _phrases_not_emitted(ids_off)
    fresh.set_boost(phrases, LOOP_BOOST)
    fresh.decode(p2, 0, want_logits=False, want_probs=False)
    ids_on, _ = fresh.decode_greedy(first, p2.shape[1], 10)
    fresh.decode(p2, 0, want_logits=False, want_probs=False)
    probs = torch.empty((batch, V), dtype=torch.float32, device="cuda")
    history, tokens = [[] for _ in range(batch)], first[:, None]
    for s in range(10):
        logits, _ = fresh.decode(tokens, p2.shape[1] + s, want_probs=False)
        boosted = dev(np.stack([R.apply(logits[b], phrases, history[b], sp["eot"], LOOP_BOOST) for b in range(batch)]))
        binding.check(binding.lib().wh_op_vocab_soft_max(None, ptr(boosted), ptr(probs), batch, V))
        tok = _tokens(binding.lib().wh_op_sample_best, probs, batch, V, sp, 0, 0)
        assert np.array_equal(tok["id"], ids_on[s]), (s, tok["id"], ids_on[s])
        for b in range(batch):
            history[b].append(int(tok["id"][b]))
        tokens = tok["id"].astype(np.int32)[:, None]
    never.decode(p2, 0, want_logits=False, want_probs=False)
    assert not np.array_equal(never.decode_greedy(first, p2.shape[1], 10)[0], ids_on)
    for z in (never, ctx, fresh):
        z.close()


def test_refusals(conditioned):
    c = conditioned
    hyp = binding.HipContext(c.model, 1, hypotheses=2)
    with pytest.raises(binding.WhisperHipError):
        hyp.set_boost([[5, 6]], 1.0)                                             # the states would have to follow the beam's reorder
    hyp.set_boost(None)
    hyp.close()
    ctx = binding.HipContext(c.model, 1)
    ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)
    with pytest.raises(binding.WhisperHipError):
        ctx.set_boost([[5, 6]], 1.0)
    ctx.set_boost(None)
    ctx.set_flags(0)
    for bad in (dict(phrases=[[5, c.sp["eot"]]], boost=1.0), dict(phrases=[[5]], boost=0.0), dict(phrases=[[5]], boost=float("nan")),
                dict(phrases=[list(range(17))], boost=1.0), dict(phrases=[[i] for i in range(1025)], boost=1.0)):
        with pytest.raises(binding.WhisperHipError):
            ctx.set_boost(**bad)
    ctx.set_boost([[5, 6]], 1.0)
    with pytest.raises(binding.WhisperHipError):
        ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)                           # the exact mode while a set is held
    ctx.set_boost(None)
    ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)
    ctx.set_flags(0)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the library
# ---------------------------------------------------------------------------------------------------------------------
import subprocess  # noqa: E402

E_NOTIMPL = 0x80004001
LIB_BOOST = 8.0
TEXT_BOOST = 32.0                                                                # for phrases given as text: see the fixture


def _pcm(seconds, tone, seed):
    t = np.arange(int(seconds * 16000)) / 16000.0
    rng = np.random.default_rng(seed)
    return (0.25 * np.sin(2 * np.pi * tone * t) * (1 + 0.6 * np.sin(2 * np.pi * 2.5 * t)) + 0.05 * rng.standard_normal(len(t))).astype(np.float32)


def _key(segs):
    return [(s["t0"], s["t1"], s["text"], [t["id"] for t in s["tokens"]]) for s in segs]


def _ids(segs):
    return [t["id"] for s in segs for t in s["tokens"]]


RECORDINGS = ((40, 330, 7), (65, 440, 8), (45, 250, 9), (35, 520, 10), (50, 390, 11), (38, 300, 12))      # seconds, tone, seed


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """A conditioned model as a model file, six recordings of one to three windows, their transcripts without a set, and phrases over the model's text
    candidates that those transcripts do not hold: the siblings (2000 + 64 i + 0 .. 3) of emitted tokens. `texts` are phrases given as text: the synthetic
    vocabulary spells them letter by letter, in tokens no transcript of this model holds, so they show only under a boost above the margin its candidates
    win by (measured on this model: the transcript is the plain one up to a boost of 16, changes at 24, and reads "h heh" at 32; from 64 on no timestamp is
    sampled any more and the host loop skips every window)."""
    from whisper_amd import api
    hp = gf.hparams_for("test-d128-ml")
    ggml = gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=125)
    path = str(tmp_path_factory.mktemp("boost") / "cond.bin")
    gf.write_model(path, ggml)
    model = api.Model(path)
    pcms = [_pcm(*r) for r in RECORDINGS]
    kw = dict(language="en", prompt=[1000], n_max_text_ctx=0, flags=api.NO_CONTEXT)
    ctx = model.create_context()
    plain = []
    for pcm in pcms:
        assert ctx.run_full(pcm, **kw) == 0
        plain.append(_key(ctx.results()))
    emitted = {t for k in plain for seg in k for t in seg[3]}
    slots = sorted({(t - 2000) // 64 for t in emitted if 2000 <= t < 2000 + 64 * 16 and (t - 2000) % 64 < 4})
    free = {i: [2000 + 64 * i + j for j in range(4) if 2000 + 64 * i + j not in emitted] for i in slots}
    chain = [free[i][0] for i in slots if free[i]]
    assert len(chain) >= 4
    phrases = [chain[0:3], chain[1:4]] + [[t] for i in slots for t in free[i][-1:]]
    texts = ["hello", "big zebra"]
    yield SimpleNamespace(api=api, path=path, model=model, pcms=pcms, kw=kw, ctx=ctx, plain=plain, phrases=phrases, texts=texts)
    ctx.close()
    model.close()


def test_library_context(library):
    """Context.set_boost_phrases with id lists: run_full and run_streamed each emit boosted tokens, which their plain transcripts do not hold, and differ from
    their plain transcripts; strings give what their spellings give as id lists, in run_full and (the phrases' letters appear) in run_streamed. With set_fallback forcing every window through all attempts (the last at temperature 1.0) the boosted run repeats, is
    the one a fresh context gives and differs from the run without a set. Beam search with a set held is E_NOTIMPL and runs once the set is cleared; cleared,
    the transcripts are the plain ones."""
    lb = library
    boosted = {t for p in lb.phrases for t in p}
    sp = lb.model.special_tokens()
    plain_streamed = []                                                          # a streamed run normalises each window on its own: its own plain transcripts
    for pcm in lb.pcms:
        hr, _ = lb.ctx.run_streamed(pcm, **lb.kw)
        assert hr == 0
        plain_streamed.append(_key(lb.ctx.results()))
    tokens_of = lambda keys: {t for k in keys for seg in k for t in seg[3]}
    assert not boosted & tokens_of(plain_streamed) and not boosted & tokens_of(lb.plain)
    lb.ctx.set_boost_phrases(lb.phrases, LIB_BOOST)
    try:
        changed, got_ids, changed_streamed, streamed_ids = 0, [], 0, []
        for pcm, off, off_streamed in zip(lb.pcms, lb.plain, plain_streamed):
            assert lb.ctx.run_full(pcm, **lb.kw) == 0
            got = lb.ctx.results()
            got_ids.append(_key(got))
            changed += int(_key(got) != off)
            hr, _ = lb.ctx.run_streamed(pcm, **lb.kw)
            assert hr == 0 and len(lb.ctx.results()) >= 1
            streamed_ids.append(_key(lb.ctx.results()))
            changed_streamed += int(streamed_ids[-1] != off_streamed)
        print("set held: %d run_full and %d run_streamed transcripts of %d differ from the plain ones" % (changed, changed_streamed, len(lb.plain)))
        assert changed >= 1 and boosted & tokens_of(got_ids)
        assert changed_streamed >= 1 and boosted & tokens_of(streamed_ids)         # the set reached the streamed runs too
        # strings: each text's two spellings, which the same call with id lists must equal
        texts = lb.texts
        rows = [r for s in texts for r in lb.model.phrase_spellings(s)]
        assert len(rows) == 2 * len(texts) and all(lb.model.tokenize(s) in rows and lb.model.tokenize(" " + s) in rows for s in texts)
        lb.ctx.set_boost_phrases(rows, TEXT_BOOST)
        assert lb.ctx.run_full(lb.pcms[0], **lb.kw) == 0
        by_ids = _key(lb.ctx.results())
        lb.ctx.set_boost_phrases(texts, TEXT_BOOST)
        assert lb.ctx.run_full(lb.pcms[0], **lb.kw) == 0
        letters = {t for r in rows for t in r}
        assert _key(lb.ctx.results()) == by_ids and by_ids != lb.plain[0] and len(by_ids) >= 1
        assert letters & {t for seg in by_ids for t in seg[3]}                    # the phrases' letters reached the transcript
        hr, _ = lb.ctx.run_streamed(lb.pcms[0], **lb.kw)
        streamed = _key(lb.ctx.results())
        assert hr == 0 and streamed != plain_streamed[0] and letters & tokens_of([streamed]) and not letters & tokens_of(plain_streamed[:1])
        with pytest.raises(ValueError):
            lb.ctx.set_boost_phrases(texts)                                      # no default boost
        # the fallback's sampled attempts: six per window, each a window start of its own, and a window start empties every history (the compute layer's
        # test_off_means_off_and_a_window_inherits_nothing). Here: the run is the one a fresh context gives, whose states no earlier attempt has touched, it
        # repeats, and it is not the run without a set
        fb = dict(temperature_inc=0.2, logprob_thold=1.0, entropy_thold=-1.0, no_speech_thold=2.0, seed=5)
        fresh = lb.model.create_context()
        fresh.set_fallback(**fb)
        lb.ctx.set_boost_phrases(lb.phrases, LIB_BOOST)
        lb.ctx.set_fallback(**fb)
        differs = 0
        for pcm in lb.pcms[:2]:
            assert fresh.run_full(pcm, **lb.kw) == 0
            unboosted = _key(fresh.results())
            assert lb.ctx.run_full(pcm, **lb.kw) == 0
            got, stats = _key(lb.ctx.results()), lb.ctx.window_stats()
            assert len(stats) >= 1 and all(w["attempts"] == 6 and w["temperature"] == 1.0 for w in stats) and len(got) >= 1
            assert lb.ctx.run_full(pcm, **lb.kw) == 0 and _key(lb.ctx.results()) == got
            differs += int(got != unboosted)
        fresh.set_boost_phrases(lb.phrases, LIB_BOOST)
        assert fresh.run_full(lb.pcms[1], **lb.kw) == 0 and _key(fresh.results()) == got and differs >= 1
        fresh.close()
        lb.ctx.set_fallback(None)
        lb.ctx.set_boost_phrases(lb.phrases, LIB_BOOST)
        with pytest.raises(lb.api.WhisperError) as e:
            lb.ctx.run_full(lb.pcms[0], beam_width=2, **lb.kw)
        assert e.value.hr == E_NOTIMPL
    finally:
        lb.ctx.set_fallback(None)
        lb.ctx.set_boost_phrases(None)
    assert lb.ctx.run_full(lb.pcms[0], beam_width=2, **lb.kw) == 0 and len(lb.ctx.results()) >= 1
    lb.ctx.set_boost_phrases([])
    for pcm, off in zip(lb.pcms[:2], lb.plain):
        assert lb.ctx.run_full(pcm, **lb.kw) == 0 and _key(lb.ctx.results()) == off
    # refusals through the library
    for bad in (dict(phrases=[[5, sp["eot"]]], boost=1.0), dict(phrases=[[5]], boost=0.0), dict(phrases=[[5]], boost=-2.0), dict(phrases=[[5]], boost=float("nan")),
                dict(phrases=[[5]], boost=float("inf")), dict(phrases=[list(range(17))], boost=1.0), dict(phrases=[[i] for i in range(1025)], boost=1.0)):
        with pytest.raises(lb.api.WhisperError):
            lb.ctx.set_boost_phrases(**bad)


def test_library_batch_runner(library):
    """BatchRunner.set_boost_phrases with 5 slots and 6 streams, the fallback on with a threshold midway between the streams' worst windows, so that some rows
    retry while their neighbours do not: every stream's transcript -- times, text, ids -- equals Context.run_full of that stream with the same set and the
    same fallback (the runner's seed for stream i is seed + i). Cleared again: the transcripts of a runner that never made the call."""
    lb = library
    kw = dict(lb.kw, flags=lb.api.NO_CONTEXT | lb.api.SINGLE_SEGMENT)
    runner = lb.model.create_batch_runner(max_slots=5, groups=1)
    hr, never, per = runner.run(lb.pcms, **kw)
    assert hr == 0 and all(p == 0 for p in per)
    never = [_key(s) for s in never]
    runner.set_boost_phrases(lb.phrases, LIB_BOOST)
    runner.set_fallback(logprob_thold=-1e30, entropy_thold=-1.0, no_speech_thold=2.0)
    hr, first, _ = runner.run(lb.pcms, **kw)
    assert hr == 0 and [_key(s) for s in first] != never
    lowest = sorted((min(x["avg_logprob"] for x in w), i) for i, w in enumerate(runner.window_stats))
    mid = len(lowest) // 2
    thold = 0.5 * (lowest[mid - 1][0] + lowest[mid][0])
    fb = dict(temperature_inc=0.5, logprob_thold=thold, entropy_thold=-1.0, no_speech_thold=2.0)
    runner.set_fallback(seed=9, **fb)
    hr, got, per = runner.run(lb.pcms, **kw)
    stats = runner.window_stats
    assert hr == 0 and all(p == 0 for p in per)
    assert any(x["attempts"] > 1 for w in stats for x in w) and any(all(x["attempts"] == 1 for x in w) for w in stats)
    lb.ctx.set_boost_phrases(lb.phrases, LIB_BOOST)
    try:
        for i, (pcm, g) in enumerate(zip(lb.pcms, got)):
            lb.ctx.set_fallback(seed=9 + i, **fb)
            assert lb.ctx.run_full(pcm, **kw) == 0
            assert _key(g) == _key(lb.ctx.results()), i
            assert [x["attempts"] for x in lb.ctx.window_stats()] == [x["attempts"] for x in stats[i]], i
    finally:
        lb.ctx.set_fallback(None)
        lb.ctx.set_boost_phrases(None)
    runner.set_fallback(None)
    runner.set_boost_phrases(None)
    hr, back, _ = runner.run(lb.pcms, **kw)
    assert hr == 0 and [_key(s) for s in back] == never
    runner.close()


def test_whisper_main_takes_the_options(library, tmp_path):
    """whisper-main --boost-phrases FILE --boost N writes the transcript of the library run with the file's phrases as strings; each option alone is refused;
    -h mentions neither."""
    import wave
    from whisper_amd import build
    lb = library
    texts = lb.texts
    phrases = str(tmp_path / "phrases.txt")
    with open(phrases, "w", encoding="utf-8") as f:
        f.write("\n".join(texts[:1] + [""] + texts[1:]) + "\n")
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
    ctx.set_boost_phrases(texts, TEXT_BOOST)
    assert ctx.run_full(pcm) == 0
    want = [s["text"] for s in ctx.results()]
    ctx.close()

    def tool(*extra, rc=0):
        r = subprocess.run([build.CLI_BIN, "-m", lb.path, "-f", wav, "-l", "en", "-nc"] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == rc, r.stderr.decode(errors="replace")[-2000:]
        return [ln.split(b"]  ", 1)[1] for ln in r.stdout.splitlines() if b"]  " in ln]

    assert tool("--boost-phrases", phrases, "--boost", str(TEXT_BOOST)) == want and len(want) >= 1 and want != plain
    tool("--boost-phrases", phrases, rc=2)
    tool("--boost", "3", rc=2)
    usage = subprocess.run([build.CLI_BIN, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "boost" not in usage.stdout + usage.stderr
