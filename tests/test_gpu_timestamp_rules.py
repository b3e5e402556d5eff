"""GPU tests of the timestamp rules ("Timestamp rules"). Everything is compared bit for bit; nothing here needs a tolerance.

  * wh_op_timestamp_rules step by step against the numpy restatement (tests/timestamp_rules_ref.py), which looks at the full history and keeps no record;
  * the device-side loop with the rules on against a host-in-the-loop emulation: wh_decode's unfiltered logits, masked by the restatement, sampled by the op
    entry points -- greedy, tempered, per-row in a ragged batch;
  * models on which the unfiltered loop breaks a clause: with the rules on it breaks none;
  * off means off, and a window does not inherit the records of the one before;
  * the library: Context / BatchRunner.set_timestamp_rules, the fallback's attempts, the refusals, whisper-main -tsr.
The CPU twin: tests/test_timestamp_rules_cpu.py."""
import ctypes as C
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import timestamp_rules_ref as R  # noqa: E402
from whisper_amd import binding, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

TOKEN_DT = np.dtype([("id", "<i4"), ("tid", "<i4"), ("p", "<f4"), ("pt", "<f4"), ("ptsum", "<f4")])
FIELDS = ("id", "tid", "p", "pt", "ptsum")
E_NOTIMPL = 0x80004001


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_records(a, b):
    """Every TokenData field, floats by their bits"""
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)) for k in FIELDS)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the op
# ---------------------------------------------------------------------------------------------------------------------
G = 4096                                                                         # NaN guard band, floats, before and behind the rows


def _op_step(body, rows, V, eot, beg, fed, reset, rec):
    binding.check(binding.lib().wh_op_timestamp_rules(None, body, rows, V, eot, beg, ptr(fed) if fed is not None else None, reset, ptr(rec)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows", [1, 4, 5, 9])
@pytest.mark.parametrize("V", [51864, 51865, 51866])
def test_op_step_by_step_against_the_restatement(V, rows):
    """Every history of tests/timestamp_rules_ref.histories, fed token by token, row r of a round on another history than its neighbours; fresh random logits
    with NaNs, -inf and NaN guard bands in every step. After every step: exactly the restatement's columns are -inf, every other float -- the guards
    included -- keeps its bits. 51864 is the synthetic .en layout, 51865 the multilingual one (the test models' and the real checkpoints'), 51866 large-v3's:
    eot, beg and the row starts are no multiples of 4 or 64. A reset launch writes no logit; an armed record folds nothing; a second reset forgets."""
    sp = gf.special_tokens(SimpleNamespace(n_vocab=V))
    eot, beg = sp["eot"], sp["beg"]
    seqs = [h for h in R.histories(eot, beg, V).values() if h]
    steps = 1 + max(len(s) for s in seqs)
    # every sequence ends on a text token and a timestamp of its own, so all rows run the same number of steps
    seqs = [(s + [777 + i] * steps)[:steps - 1] + [min(V - 1, max([beg + 5] + [t for t in s if t >= beg]) + i % 3)] for i, s in enumerate(seqs)]
    rng = np.random.default_rng(V * 16 + rows)
    rec = torch.full((rows, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")     # garbage: the reset must not depend on what was there
    n_masked = 0

    def fresh():
        flat = np.full(G + rows * V + G, np.nan, np.float32)
        flat.view(np.uint32)[:G] = 0x7FC00123                                    # NaNs with a payload: a rewritten guard would lose it
        flat.view(np.uint32)[-G:] = 0x7FC00321
        x = (3.0 * rng.standard_normal((rows, V))).astype(np.float32)
        x[rows - 1, rng.integers(0, V, 300)] = -np.inf
        x[0, rng.integers(0, V, 40)] = np.nan
        flat[G:G + rows * V] = x.ravel()
        buf = dev(flat)
        return flat, buf, C.c_void_p(buf.data_ptr() + 4 * G)

    def check_step(histories, fed, reset=0):
        nonlocal n_masked
        flat, buf, body = fresh()
        _op_step(body, rows, V, eot, beg, dev(np.asarray(fed, np.int32)) if fed is not None else None, reset, rec)
        want = flat.copy()
        w = want[G:G + rows * V].reshape(rows, V)
        for r, h in enumerate(histories):
            m = R.mask(h, eot, beg, V)
            w[r, m] = -np.inf
            n_masked += int(m.sum())
        assert np.array_equal(buf.cpu().numpy().view(np.uint32), want.view(np.uint32)), (V, rows, histories)

    for start in range(0, len(seqs), rows):
        mine = [seqs[(start + r) % len(seqs)] for r in range(rows)]
        check_step([[]] * rows, None, reset=1)                                   # the prompt step: nothing is masked, whatever the records held
        for k in range(steps):
            check_step([s[:k + 1] for s in mine], [s[k] for s in mine])
    assert n_masked > 0
    # a second reset returns to "mask nothing": armed, the fed token is not a sample and the history stays empty; then a history from scratch
    mine = [seqs[r % len(seqs)] for r in range(rows)]
    check_step([[]] * rows, None, reset=2)
    check_step([[]] * rows, [beg + 9] * rows)
    check_step([[s[0]] for s in mine], [s[0] for s in mine])
    check_step([[]] * rows, None, reset=1)
    check_step([[s[1]] for s in mine], [s[1] for s in mine])
    got = rec.cpu().numpy()
    assert (got[:, 3] == 1).all()                                                # one token sampled since the reset
    # bad arguments
    L = binding.lib()
    x, i = dev(np.zeros(16, np.float32)), dev(np.zeros(4, np.int32))
    assert L.wh_op_timestamp_rules(None, None, 1, 16, 2, 8, ptr(i), 0, ptr(i)) != 0 and L.wh_op_timestamp_rules(None, ptr(x), 0, 16, 2, 8, ptr(i), 0, ptr(i)) != 0
    assert L.wh_op_timestamp_rules(None, ptr(x), 1, 16, 2, 8, None, 0, ptr(i)) != 0 and L.wh_op_timestamp_rules(None, ptr(x), 1, 16, 2, 8, ptr(i), 0, None) != 0
    assert L.wh_op_timestamp_rules(None, ptr(x), 1, 16, 8, 8, ptr(i), 0, ptr(i)) != 0 and L.wh_op_timestamp_rules(None, ptr(x), 1, 16, 2, 16, ptr(i), 0, ptr(i)) != 0
    assert L.wh_op_timestamp_rules(None, ptr(x), 1, 16, 0, 0, ptr(i), 0, ptr(i)) != 0 and L.wh_op_timestamp_rules(None, ptr(x), 1, 16, 2, 8, ptr(i), 3, ptr(i)) != 0
    assert L.wh_op_timestamp_rules(None, ptr(x), 1, 16, 2, 8, None, 1, ptr(i)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. the device-side loop against a host-in-the-loop emulation
# ---------------------------------------------------------------------------------------------------------------------
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


def _tokens(fn, probs_dev, rows, V, sp, force, initial, extra=()):
    out = torch.zeros(rows * 5, dtype=torch.int32, device="cuda")
    binding.check(fn(None, ptr(probs_dev), rows, V, sp["beg"], sp["sot"], sp["solm"], sp["not_"], int(force), int(initial), *extra, ptr(out)))
    torch.cuda.synchronize()
    return np.frombuffer(out.cpu().numpy().tobytes(), TOKEN_DT)


def _emulate(ctx, prompt, n_steps, sp, V, temperature=0.0, seed=0, nonce=0):
    """wh_decode (unfiltered, whatever mode the context is in) -> the restatement's mask on the host -> the op entry points pick the token. Returns the records
    [1 + n_steps][batch]."""
    L = binding.lib()
    batch, n_prompt = prompt.shape
    probs = torch.empty((batch, V), dtype=torch.float32, device="cuda")
    history = [[] for _ in range(batch)]
    tokens, n_past, out = prompt, 0, []
    for s in range(1 + n_steps):
        logits, _ = ctx.decode(tokens, n_past, want_probs=False)
        assert np.isfinite(logits).all()                                         # wh_decode is unfiltered
        masked = np.stack([R.apply(logits[b], history[b], sp["eot"], sp["beg"]) for b in range(batch)])
        first = int(s == 0)
        x = dev(masked)
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
    """wh_decode_window_start plus chunks with the rules on, 20 steps, at 1, 4 and 5 rows (the single-stream decode path and the batched one), greedy and at
    temperature 0.8 through wh_context_set_sampling, graph replay and eager steps: token for token and bit for bit in p / pt / ptsum what the emulation gives.
    The rules must matter here: the run differs from the one with the rules off."""
    c, sp, V = conditioned, conditioned.sp, conditioned.hp.n_vocab
    n_steps, seed, nonce = 20, 0xDEADBEEFCAFE, 24 * 8 + 3
    prompt = _prompts4(sp, batch)
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(_mels(batch))
    if temperature > 0:
        ctx.set_sampling(temperature, seed, nonce)
    off = _window(ctx, prompt, n_steps)
    ctx.set_timestamp_rules(True)
    runs = [_window(ctx, prompt, n_steps), _window(ctx, prompt, n_steps, chunk=4)]
    ctx.set_flags(binding.WH_FLAG_NO_GRAPH)
    runs.append(_window(ctx, prompt, n_steps, chunk=4))
    ctx.set_flags(0)
    for r in runs[1:]:
        assert same_records(r, runs[0])
    want = _emulate(ctx, prompt, n_steps, sp, V, temperature, seed, nonce)
    for k in FIELDS:
        assert np.array_equal(np.ascontiguousarray(runs[0][k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)), (k, runs[0][k], want[k])
    for b in range(batch):
        assert R.violations(runs[0]["id"][:, b], sp["eot"], sp["beg"], V) == []
    assert not np.array_equal(runs[0]["id"], off["id"])
    assert same_records({k: v[:1] for k, v in runs[0].items()}, {k: v[:1] for k, v in off.items()})       # the prompt step's sample is unfiltered
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
    wh_context_set_sampling_rows, the rules on, one enqueue and chunks of 4. The rows with full-length prompts (1 and 4 sampled, 3 greedy) are replayed
    through wh_decode -- the device's own tokens fed back, as tests/test_gpu_batch_fallback.py does -- the restatement's mask and the per-row op on the masked
    logits (a greedy row = wh_op_vocab_soft_max + wh_op_sample_best, a sampled row = the scaled softmax + wh_op_sample_draw: that file shows it): their
    records, bit for bit. Every row obeys the clauses."""
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
    ctx.set_timestamp_rules(True)
    on = ragged()
    assert same_records(ragged(chunk=4), on) and not np.array_equal(on["id"], off["id"])
    for b in range(batch):
        assert R.violations(on["id"][:, b], sp["eot"], sp["beg"], V) == [], b
    padded = np.zeros((batch, n_max), np.int32)
    for b, p in enumerate(prompts):
        padded[b, :len(p)] = p
    tokens, n_past = padded, 0
    for s in range(1 + n_steps):
        logits, _ = ctx.decode(tokens, n_past, want_probs=False)
        masked = np.stack([R.apply(logits[b], on["id"][:s, b], sp["eot"], sp["beg"]) for b in range(batch)])
        pos = dev(np.full(batch, n_max - 1 + s, np.int32))
        first = int(s == 0)
        tok = _sample_rows(dev(masked), batch, V, sp, first, first, temps, seeds, nonces, pos)
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


@pytest.mark.parametrize("model_seed", [114, 20])
def test_a_window_that_breaks_a_clause_obeys_them_all_with_the_rules_on(model_seed):
    """How the seeds were found: on the CPU, oracle/whisper_np.py (WhisperNP.decode with exact_pv = False, sample_best with the forced initial timestamp on
    the first sample) decoded 20 steps of conditioned_model( conditioned_layout, 4, "test-d128-ml", seed ) for seeds 1 .. 120 behind the prompt
    [prev, 1000, sot, sot + 1] on uniform( -1, 1 ) mel rows (generator seed 17), and tests/timestamp_rules_ref.violations read each sequence up to its eot.
    23 of the 120 seeds break a clause before eot. Seed 114 is the one that goes BACK IN TIME: <|8.66|> then <|7.32|> at samples 6 and 7 -- the case the
    host loop answers by cutting the window. Seed 20 holds six timestamps in a row at samples 6 .. 11: the pair clause, four times.
    With the rules off the device loop must break a clause before eot on some row (asserted: the oracle is not the device). With them on, greedy and at
    temperature 1.0, two windows in a row on other audio, 5 rows: no sample of any row lies in the mask its own history gives -- through eot and beyond it,
    where the loop keeps sampling."""
    c = _conditioned(model_seed)
    sp, V = c.sp, c.hp.n_vocab
    batch, n_steps = 5, 24
    prompt = _prompts4(sp, batch)
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(_mels(batch))
    off = _window(ctx, prompt, n_steps)
    broken = {b: R.violations(_until_eot(off["id"][:, b], sp["eot"]), sp["eot"], sp["beg"], V) for b in range(batch)}
    print("model seed %d, rules off: violations before eot per row %s; row 0: %s" % (model_seed, broken, off["id"][:, 0].tolist()))
    assert any(broken.values())
    ctx.set_timestamp_rules(True)
    for temperature in (0.0, 1.0):
        ctx.set_sampling(temperature, 77, 5)
        for mel_seed in (17, 18):
            ctx.encode(_mels(batch, mel_seed))
            on = _window(ctx, prompt, n_steps, chunk=4 if mel_seed == 18 else 0)
            for b in range(batch):
                assert R.violations(on["id"][:, b], sp["eot"], sp["beg"], V) == [], (temperature, mel_seed, b, on["id"][:, b].tolist())
            stamps = [[int(t) for t in on["id"][:, b] if t >= sp["beg"]] for b in range(batch)]
            assert all(s == sorted(s) for s in stamps) and all(len(s) >= 1 for s in stamps)
    ctx.close()
    c.model.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. off means off
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [2, 5])
def test_off_means_off_and_a_window_inherits_nothing(conditioned, batch):
    """On and off again: the records of a window -- tokens, ptsum and every other field, bit for bit -- are those of a context that never made the call.
    With the rules on, a second window behind a first one equals that window on a context that never saw the first: no record survives the prompt step.
    wh_decode_greedy counts from its own first sample: firstTokens, a timestamp, is not taken for a sampled one."""
    c, sp, V = conditioned, conditioned.sp, conditioned.hp.n_vocab
    n_steps = 16
    p1, p2 = _prompts4(sp, batch), _prompts4(sp, batch) + np.array([0, 13, 0, 0], np.int32)
    never = binding.HipContext(c.model, batch)
    never.encode(_mels(batch))
    base = _window(never, p1, n_steps)
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(_mels(batch))
    assert same_records(_window(ctx, p1, n_steps), base)
    ctx.set_timestamp_rules(True)
    on1 = _window(ctx, p1, n_steps)
    ctx.encode(_mels(batch, 18))
    on2 = _window(ctx, p2, n_steps)                                              # behind window 1, whose records end in other states
    ctx.set_timestamp_rules(False)
    ctx.encode(_mels(batch))
    assert same_records(_window(ctx, p1, n_steps), base) and not same_records(on1, base)
    assert same_records(_window(never, p1, n_steps), base)
    fresh = binding.HipContext(c.model, batch)
    fresh.set_timestamp_rules(True)
    fresh.encode(_mels(batch, 18))
    assert same_records(_window(fresh, p2, n_steps), on2)
    # wh_decode_greedy: behind a prompt fed by wh_decode, firstTokens = the LAST timestamp of the vocabulary. Were it counted as a sample, every timestamp
    # below it would be masked for the rest of the call and none could follow; the model's layout has two at samples 5 and 6. The first sample is the one a
    # context without the rules gives, and the samples behind it obey the clauses with the history starting there
    first = np.full(batch, V - 1, np.int32)
    fresh.decode(p2, 0, want_logits=False, want_probs=False)
    ids_on, _ = fresh.decode_greedy(first, p2.shape[1], 12)
    never.encode(_mels(batch, 18))
    never.decode(p2, 0, want_logits=False, want_probs=False)
    ids_off, _ = never.decode_greedy(first, p2.shape[1], 12)
    assert np.array_equal(ids_on[0], ids_off[0])
    for b in range(batch):
        assert R.violations(ids_on[:, b], sp["eot"], sp["beg"], V) == []
        assert ((ids_on[:, b] >= sp["beg"]) & (ids_on[:, b] < V - 1)).any(), ids_on[:, b].tolist()
    for x in (never, ctx, fresh):
        x.close()


def test_refusals(conditioned):
    c = conditioned
    hyp = binding.HipContext(c.model, 1, hypotheses=2)
    with pytest.raises(binding.WhisperHipError):
        hyp.set_timestamp_rules(True)                                            # the records would have to follow the beam's reorder
    hyp.set_timestamp_rules(False)
    hyp.close()
    ctx = binding.HipContext(c.model, 1)
    ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)
    with pytest.raises(binding.WhisperHipError):
        ctx.set_timestamp_rules(True)
    ctx.set_timestamp_rules(False)
    ctx.set_flags(0)
    ctx.set_timestamp_rules(True)
    with pytest.raises(binding.WhisperHipError):
        ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)                           # the exact mode while the rules are on
    ctx.set_timestamp_rules(False)
    ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)
    ctx.set_flags(0)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the library
# ---------------------------------------------------------------------------------------------------------------------
def _pcm(seconds, tone, seed):
    t = np.arange(int(seconds * 16000)) / 16000.0
    rng = np.random.default_rng(seed)
    return (0.25 * np.sin(2 * np.pi * tone * t) * (1 + 0.6 * np.sin(2 * np.pi * 2.5 * t)) + 0.05 * rng.standard_normal(len(t))).astype(np.float32)


def _key(segs):
    return [(s["t0"], s["t1"], s["text"], [t["id"] for t in s["tokens"]]) for s in segs]


def _ordered(segs):
    """t0 <= t1 in every segment, and the segments non-decreasing: neither a begin nor an end lies before the one of the segment in front of it. (A window's
    next seek is its last timestamp's id, a segment's end the most probable timestamp `tid`, as in the reference: under sampling the two may differ, so a
    window's first segment may begin before the end the last one shows. That is the host loop's, and not a disorder.)"""
    times = [(s["t0"], s["t1"]) for s in segs]
    return all(a <= b for a, b in times) and all(times[i][0] <= times[i + 1][0] and times[i][1] <= times[i + 1][1] for i in range(len(times) - 1))


RECORDINGS = ((40, 330, 7), (65, 440, 8), (45, 250, 9), (35, 520, 10), (50, 390, 11), (38, 300, 12))      # seconds, tone, seed


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """A model that goes back in time on the first window of the first recording -- found like the seeds above, the oracle fed the log-mel spectrogram of
    _pcm( 40, 330, 7 ): seed 125 samples <|7.32|> and then <|6.00|>, the case the host loop answers by cutting the window -- as a model file, and six
    recordings of one to three windows"""
    from whisper_amd import api
    hp = gf.hparams_for("test-d128-ml")
    ggml = gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=125)
    path = str(tmp_path_factory.mktemp("tsr") / "cond.bin")
    gf.write_model(path, ggml)
    model = api.Model(path)
    pcms = [_pcm(*r) for r in RECORDINGS]
    kw = dict(language="en", prompt=[1000], n_max_text_ctx=0, flags=api.NO_CONTEXT)
    ctx = model.create_context()
    yield SimpleNamespace(api=api, path=path, model=model, pcms=pcms, kw=kw, ctx=ctx)
    ctx.close()
    model.close()


def test_library_context(library):
    """Context.set_timestamp_rules: run_full and run_streamed give ordered segments on every recording; off again the transcripts are those of a context
    that never made the call; with set_fallback forcing every window through all attempts (the last at temperature 1.0) the sampled attempts are ordered
    too. Beam search with the rules on is E_NOTIMPL, and runs once they are off."""
    lb = library
    fresh = lb.model.create_context()
    plain = []
    for pcm in lb.pcms:
        assert fresh.run_full(pcm, **lb.kw) == 0
        plain.append(_key(fresh.results()))
    lb.ctx.set_timestamp_rules(True)
    try:
        changed = 0
        for pcm, off in zip(lb.pcms, plain):
            assert lb.ctx.run_full(pcm, **lb.kw) == 0
            got = lb.ctx.results()
            assert len(got) >= 1 and _ordered(got), [(s["t0"], s["t1"]) for s in got]
            changed += int(_key(got) != off)
            hr, _ = lb.ctx.run_streamed(pcm, **lb.kw)
            assert hr == 0 and _ordered(lb.ctx.results()) and len(lb.ctx.results()) >= 1
        print("rules on: %d of %d transcripts differ from the unfiltered ones" % (changed, len(plain)))
        assert changed >= 1                                                      # the rules reached the transcripts
        lb.ctx.set_fallback(temperature_inc=0.2, logprob_thold=1.0, entropy_thold=-1.0, no_speech_thold=2.0, seed=5)
        for pcm in lb.pcms[:3]:
            assert lb.ctx.run_full(pcm, **lb.kw) == 0
            got, stats = lb.ctx.results(), lb.ctx.window_stats()
            assert len(stats) >= 1 and all(w["attempts"] == 6 and w["temperature"] == 1.0 for w in stats)
            assert len(got) >= 1 and _ordered(got), [(s["t0"], s["t1"]) for s in got]
        lb.ctx.set_fallback(None)
        with pytest.raises(lb.api.WhisperError) as e:
            lb.ctx.run_full(lb.pcms[0], beam_width=2, **lb.kw)
        assert e.value.hr == E_NOTIMPL
    finally:
        lb.ctx.set_fallback(None)
        lb.ctx.set_timestamp_rules(False)
    assert lb.ctx.run_full(lb.pcms[0], beam_width=2, **lb.kw) == 0 and len(lb.ctx.results()) >= 1
    for pcm, off in zip(lb.pcms[:2], plain):
        assert lb.ctx.run_full(pcm, **lb.kw) == 0 and _key(lb.ctx.results()) == off
    fresh.close()


def test_library_batch_runner(library):
    """BatchRunner.set_timestamp_rules with 5 slots and 6 streams, the fallback on with a threshold midway between the streams' worst windows, so that some
    rows retry while their neighbours do not: every stream's transcript -- times, text, ids -- equals Context.run_full of that stream with the rules on and
    the same fallback (the runner's seed for stream i is seed + i), and is ordered. Off again: the transcripts of a runner that never made the call."""
    lb = library
    kw = dict(lb.kw, flags=lb.api.NO_CONTEXT | lb.api.SINGLE_SEGMENT)
    runner = lb.model.create_batch_runner(max_slots=5, groups=1)
    hr, never, per = runner.run(lb.pcms, **kw)
    assert hr == 0 and all(p == 0 for p in per)
    never = [_key(s) for s in never]
    runner.set_timestamp_rules(True)
    runner.set_fallback(logprob_thold=-1e30, entropy_thold=-1.0, no_speech_thold=2.0)
    hr, _, _ = runner.run(lb.pcms, **kw)
    lowest = sorted((min(x["avg_logprob"] for x in w), i) for i, w in enumerate(runner.window_stats))
    mid = len(lowest) // 2
    thold = 0.5 * (lowest[mid - 1][0] + lowest[mid][0])
    fb = dict(temperature_inc=0.5, logprob_thold=thold, entropy_thold=-1.0, no_speech_thold=2.0)
    runner.set_fallback(seed=9, **fb)
    hr, got, per = runner.run(lb.pcms, **kw)
    stats = runner.window_stats
    assert hr == 0 and all(p == 0 for p in per)
    assert any(x["attempts"] > 1 for w in stats for x in w) and any(all(x["attempts"] == 1 for x in w) for w in stats)
    lb.ctx.set_timestamp_rules(True)
    try:
        for i, (pcm, g) in enumerate(zip(lb.pcms, got)):
            lb.ctx.set_fallback(seed=9 + i, **fb)
            assert lb.ctx.run_full(pcm, **kw) == 0
            assert _key(g) == _key(lb.ctx.results()), i
            assert [x["attempts"] for x in lb.ctx.window_stats()] == [x["attempts"] for x in stats[i]], i
            assert _ordered(g) and len(g) >= 1, i
    finally:
        lb.ctx.set_fallback(None)
        lb.ctx.set_timestamp_rules(False)
    runner.set_fallback(None)
    runner.set_timestamp_rules(False)
    hr, back, _ = runner.run(lb.pcms, **kw)
    assert hr == 0 and [_key(s) for s in back] == never
    runner.close()


def test_whisper_main_takes_the_option(library, tmp_path):
    """whisper-main -tsr / --timestamp-rules writes the transcript of the library run with the rules on; -h does not mention the option."""
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
    ctx.set_timestamp_rules(True)
    assert ctx.run_full(pcm) == 0
    texts = [s["text"] for s in ctx.results()]
    ctx.close()

    def tool(*extra):
        r = subprocess.run([build.CLI_BIN, "-m", lb.path, "-f", wav, "-l", "en", "-nc"] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        return [ln.split(b"]  ", 1)[1] for ln in r.stdout.splitlines() if b"]  " in ln]

    assert tool("-tsr") == texts and tool("--timestamp-rules") == texts and len(texts) >= 1
    usage = subprocess.run([build.CLI_BIN, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "-tsr" not in usage.stdout + usage.stderr and "timestamp-rules" not in usage.stdout + usage.stderr
