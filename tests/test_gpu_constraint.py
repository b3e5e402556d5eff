"""GPU tests of constrained decoding ("Constrained decoding"): the two kernels and the device-side loop against tests/constraint_ref.py.
Everything is compared exactly -- words, states, ids, and floats by their bits: the arithmetic is integer apart from one FP32 subtraction per entry."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import constraint_ref as R  # noqa: E402
import test_gpu_timestamp_rules as T  # noqa: E402  (its helpers: windows, the samplers' op entry points)
from whisper_amd import binding, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu
dev, ptr, same_records, FIELDS = T.dev, T.ptr, T.same_records, T.FIELDS
G, GUARD = 1024, 0xA5C3A5C3                                                      # guard band, elements, before and behind a buffer, and what it holds


def _random_constraint(rng, n_states, n_classes, eot, missing, lengths):
    trans = rng.integers(0, n_states, (n_states, n_classes)).astype(np.int32)
    trans[rng.random((n_states, n_classes)) < missing] = -1
    offsets = np.concatenate([[0], np.cumsum(rng.choice(lengths, eot))]).astype(np.int32)
    data = rng.integers(0, 256, int(offsets[-1]) + 1).astype(np.uint8)           # one byte behind the last token: never an empty upload
    return rng.integers(0, n_classes, 256).astype(np.uint8), trans, rng.integers(0, 2, n_states).astype(np.uint8), offsets, data


def _tables(class_of, trans, accept, offsets, data, start=0):
    """wh_constraint_tables over device copies (kept alive by the caller through the returned list)"""
    keep = [dev(class_of), dev(trans), dev(accept), dev(offsets), dev(data)]
    return binding.ConstraintTablesC(trans.shape[0], trans.shape[1], start, len(offsets) - 1, *[k.data_ptr() for k in keep], int(offsets[-1])), keep


@pytest.mark.parametrize("n_states,n_classes", [(1, 1), (1, 7), (1, 256), (2, 1), (2, 7), (2, 256), (65, 1), (65, 7), (65, 256), (300, 1), (300, 7), (256, 256)])
def test_mask_kernel_equals_the_reference_walk(n_states, n_classes):
    """allowed[ s ][ t / 32 ] of random automata -- half of the transitions missing, and 2 % so that long walks survive -- over vocabularies of 1, 63, 64, 65 and
    200 tokens of 0, 1, 2, 5, 17 and 255 bytes: a tail inside the first wave, a whole wave, one token into the second, more words than one; one state tile and
    several; the table at its 65536-entry limit (256 x 256). Every word equals the reference's, absent tokens' bits are 0 (the buffer is all ones before), and the
    guard words around the buffer keep their value."""
    rng = np.random.default_rng(1000 * n_states + n_classes)
    for eot in (1, 63, 64, 65, 200):
        for missing in (0.5, 0.02):
            con = _random_constraint(rng, n_states, n_classes, eot, missing, [0, 1, 2, 5, 17, 255])
            want = R.allowed_words(con[0], con[1], con[3], con[4], eot)
            n = want.size
            flat = np.full(G + n + G, GUARD, np.uint32)
            flat[G:G + n] = 0xFFFFFFFF
            buf = dev(flat)
            t, keep = _tables(*con)
            binding.check(binding.lib().wh_op_constraint_mask(None, C.byref(t), C.c_void_p(buf.data_ptr() + 4 * G)))
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert np.array_equal(got[G:G + n].reshape(want.shape), want), (eot, missing)
            assert (got[:G] == GUARD).all() and (got[G + n:] == GUARD).all(), (eot, missing)
            if n_states * n_classes == 1 and con[1][0, 0] == 0:
                assert want.any()                                                # the 255-byte tokens survive here: the reload path decides bits


@pytest.mark.parametrize("n_states", [500, 1000, 2000, 4096])
def test_mask_kernel_at_every_state_tile(n_states):
    """16001 tokens are 16 workgroups along the vocabulary, where the launcher gives 500, 1000, 2000 and 4096 states tiles of 16, 32, 64 and 128 states (the
    cases above all run at 8): another split of LDS between the output words and the table, several rounds of the write-out loop, blockIdx.x above 0, and at
    4096 x 16 the full 144 KB. Every word against the reference."""
    rng = np.random.default_rng(n_states)
    con = _random_constraint(rng, n_states, 16, 16001, 0.1, [0, 1, 2, 5, 17])
    want = R.allowed_words(con[0], con[1], con[3], con[4], 16001)
    buf = dev(np.full(G + want.size + G, GUARD, np.uint32))
    t, keep = _tables(*con)
    binding.check(binding.lib().wh_op_constraint_mask(None, C.byref(t), C.c_void_p(buf.data_ptr() + 4 * G)))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[G:-G].reshape(want.shape), want) and (got[:G] == GUARD).all() and (got[-G:] == GUARD).all()


@pytest.mark.parametrize("penalty", [100.0, float("inf")])
@pytest.mark.parametrize("rows", [1, 3, 70])
def test_apply_kernel_states_and_rows_bit_for_bit(rows, penalty):
    """One step on rows whose states cycle through start, an accepting state, a non-accepting one and -1, fed a text token whose walk survives, one whose walk
    dies and an id >= eot; rows of random floats with -inf entries between guard bands, eot = 203 in rows of 233 floats (no row start, and no line of
    `allowed`, at a multiple of 16 bytes but the first). The new states, and every float -- the columns above eot and the guards included -- by their bits.
    Then the two resets: states only, no float changes; and an armed state becomes start whatever is fed."""
    rng = np.random.default_rng(rows)
    eot, V, n_states, start = 203, 233, 12, 5
    while True:
        con = _random_constraint(rng, n_states, 5, eot, 0.3, [0, 1, 2, 5])
        class_of, trans, accept, offsets, data = con
        dead = [R.dead_tokens(class_of, trans, offsets, data, s, eot) for s in range(n_states)]
        yes, no = [s for s in range(n_states) if accept[s] and s != start], [s for s in range(n_states) if not accept[s] and s != start]
        if yes and no and all(not d.all() and d.any() for d in dead):
            break
    states = np.array([[start, yes[0], no[0], -1][r % 4] for r in range(rows)], np.int32)
    fed = np.zeros(rows, np.int32)
    for r in range(rows):
        kind, s = (r // 4) % 3, states[r]
        pick = np.flatnonzero(dead[s] == (kind == 1)) if s >= 0 else np.arange(eot)
        fed[r] = eot + r % (V - eot) if kind == 2 else int(pick[r % len(pick)])
    want_states = np.array([R.advance(class_of, trans, offsets, data, states[r], fed[r], eot) for r in range(rows)], np.int32)
    if rows >= 12:
        assert {-1, start, yes[0], no[0]} <= set(states.tolist()) and (want_states[states >= 0] == -1).any() and (want_states[fed < eot] >= 0).any()
    x = (3.0 * rng.standard_normal((rows, V))).astype(np.float32)
    x[rng.random((rows, V)) < 0.05] = -np.inf
    flat = np.full(G + rows * V + G, np.nan, np.float32)
    flat.view(np.uint32)[:G] = 0x7FC00123
    flat.view(np.uint32)[-G:] = 0x7FC00321
    flat[G:G + rows * V] = x.ravel()
    want = flat.copy()
    want[G:G + rows * V] = np.stack([R.apply(x[r], dead[want_states[r]] if want_states[r] >= 0 else np.ones(eot, bool), want_states[r], accept, eot, penalty)
                                     for r in range(rows)]).ravel()
    buf, st, fd = dev(flat), dev(states), dev(fed)
    allowed = dev(R.allowed_words(class_of, trans, offsets, data, eot))
    t, keep = _tables(*con, start=start)
    L, body = binding.lib(), C.c_void_p(buf.data_ptr() + 4 * G)
    binding.check(L.wh_op_constraint_apply(None, body, rows, V, eot, C.byref(t), ptr(allowed), ptr(st), ptr(fd), 0, penalty))
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), want_states)
    got = buf.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and not np.array_equal(got.view(np.uint32), flat.view(np.uint32))
    for reset, value in ((1, start), (2, -2)):
        binding.check(L.wh_op_constraint_apply(None, body, rows, V, eot, C.byref(t), ptr(allowed), ptr(st), None, reset, penalty))
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == value).all() and np.array_equal(buf.cpu().numpy().view(np.uint32), want.view(np.uint32))
    binding.check(L.wh_op_constraint_apply(None, body, rows, V, eot, C.byref(t), ptr(allowed), ptr(st), ptr(fd), 0, penalty))
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == start).all()


class Digits:
    """Digits and single spaces, ending on a digit: state 0 = at the start or behind a space (a digit must follow), state 1 = behind a digit. An invented
    vocabulary for the test model's ids (the compute layer takes the byte strings from the caller): a number, a space and a number, a word, a number and a space."""

    def __init__(self, eot):
        self.eot = eot
        self.class_of = np.full(256, 2, np.uint8)
        self.class_of[ord("0"):ord("9") + 1] = 0
        self.class_of[ord(" ")] = 1
        self.trans, self.accept = np.array([[1, -1, -1], [1, 0, -1]], np.int32), np.array([0, 1], np.uint8)
        words = [(str(t // 4 % 1000), " " + str(t % 10), "w" + str(t), str(t % 7) + " ")[t % 4].encode() for t in range(eot)]
        self.offsets = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int32)
        self.data = np.frombuffer(b"".join(words), np.uint8)
        self.dead = [R.dead_tokens(self.class_of, self.trans, self.offsets, self.data, s, eot) for s in (0, 1)]
        self.args = (self.class_of, self.trans, self.accept, 0, self.offsets, self.data)

    def filter(self, row, history):
        """what the loop does to the row in front of the sample behind `history`: nothing in front of the first"""
        if len(history) == 0:
            return row
        s = 0
        for t in history:
            s = R.advance(self.class_of, self.trans, self.offsets, self.data, s, int(t), self.eot)
        return R.apply(row, self.dead[s] if s >= 0 else np.ones(self.eot, bool), s, self.accept, self.eot, np.inf)

    def reads(self, ids):
        """does the automaton read the row's text, up to its eot, as a prefix"""
        ids = [int(t) for t in ids]
        ids = ids[:ids.index(self.eot)] if self.eot in ids else ids
        return R.walk_bytes(self.class_of, self.trans, 0, b"".join(R.token_bytes(self.offsets, self.data, t) for t in ids if t < self.eot)) >= 0


@pytest.fixture(scope="module")
def looping():
    hp = gf.hparams_for("test-d128-ml")
    model = binding.HipModel.from_ggml(gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=4, alpha=30.0))
    sp = gf.special_tokens(hp)
    yield hp, model, sp, Digits(sp["eot"])
    model.close()


@pytest.mark.parametrize("mode", ["greedy", "rows"])
def test_device_loop_equals_the_host_stepped_windows(looping, mode):
    """wh_decode_window_start with a digits-and-space automaton at penalty +inf, 3 rows, 12 steps, in one enqueue and in chunks of 4; greedy, and through
    wh_context_set_sampling_rows with row 1 sampled at 0.8 between two greedy rows. The records equal those of the same windows stepped from the host: wh_decode
    with the device's own tokens fed back, the reference filter on the downloaded logits, the sampler's op entry point. The text of every row is a prefix the
    automaton reads, and the unconstrained run's is not; the first sample is the unconstrained run's; a second window starts from `start` again (it equals the
    first); another automaton and penalty capture nothing new; set_constraint() gives the unconstrained records of the fresh context back."""
    hp, model, sp, dfa = looping
    V, batch, n_steps = hp.n_vocab, 3, 12
    temps, seeds, nonces = np.array([0, 0.8, 0], np.float32), np.array([1, 0xDEADBEEFCAFE, 2], np.uint64), np.array([0, 24 * 8 + 3, 0], np.uint32)
    prompt = T._prompts4(sp, batch)
    ctx = binding.HipContext(model, batch)
    ctx.encode(T._mels(batch))
    if mode == "rows":
        ctx.set_sampling_rows(temps, seeds, nonces)
    off = T._window(ctx, prompt, n_steps)
    vram = ctx.vram_bytes()
    ctx.set_constraint(*dfa.args, penalty=float("inf"))
    assert ctx.vram_bytes() > vram
    on = T._window(ctx, prompt, n_steps)
    assert same_records(T._window(ctx, prompt, n_steps), on) and same_records(T._window(ctx, prompt, n_steps, chunk=4), on)
    print(mode, "off", off["id"].T.tolist(), "on", on["id"].T.tolist())
    L, probs = binding.lib(), torch.empty((batch, V), dtype=torch.float32, device="cuda")
    tokens, n_past = prompt, 0
    for s in range(1 + n_steps):
        logits, _ = ctx.decode(tokens, n_past, want_probs=False)
        x, first = dev(np.stack([dfa.filter(logits[b], on["id"][:s, b]) for b in range(batch)])), int(s == 0)
        if mode == "rows":
            tok = T._sample_rows(x, batch, V, sp, first, first, temps, seeds, nonces, dev(np.full(batch, prompt.shape[1] - 1 + s, np.int32)))
        else:
            binding.check(L.wh_op_vocab_soft_max(None, ptr(x), ptr(probs), batch, V))
            tok = T._tokens(L.wh_op_sample_best, probs, batch, V, sp, first, first)
        assert np.array_equal(tok["id"], on["id"][s]) and same_records({k: on[k][s] for k in FIELDS}, tok), (s, tok["id"], on["id"][s])
        n_past += tokens.shape[1]
        tokens = on["id"][s].astype(np.int32)[:, None].copy()
    assert same_records({k: v[:1] for k, v in on.items()}, {k: v[:1] for k, v in off.items()})
    assert all(dfa.reads(on["id"][:, b]) for b in range(batch)) and not all(dfa.reads(off["id"][:, b]) for b in range(batch))
    captures = ctx.step_captures()
    ctx.set_constraint(dfa.class_of, np.array([[0, 0, -1]], np.int32), np.array([1], np.uint8), 0, dfa.offsets, dfa.data, penalty=100.0)
    T._window(ctx, prompt, n_steps)
    assert ctx.step_captures() == captures
    ctx.set_constraint()
    assert same_records(T._window(ctx, prompt, n_steps), off)
    ctx.close()


def test_refusals_that_need_the_device(looping):
    """What the host's option rules (tests/test_constraint_cpu.py) cannot see: a vocabulary that is not the model's, a token of more than 255 bytes, a limit at the
    compute layer's own check, WH_FLAG_PARITY_EXACT in both orders of setting, a hypothesis-group context."""
    hp, model, sp, dfa = looping
    ctx = binding.HipContext(model, 1)
    names = ("class_of", "trans", "accept", "start", "tok_offsets", "tok_bytes")
    long = dfa.offsets.copy()
    long[1:] += 256
    for word, kw in (("nTokens", dict(tok_offsets=dfa.offsets[:-1])), ("255", dict(tok_offsets=long, tok_bytes=np.zeros(int(long[-1]), np.uint8))),
                     ("65536", dict(trans=np.zeros((300, 256), np.int32), accept=np.zeros(300, np.uint8))), ("penalty", dict(penalty=float("nan")))):
        with pytest.raises(binding.WhisperHipError, match=word):
            ctx.set_constraint(**{**dict(zip(names, dfa.args), penalty=100.0), **kw})
    ctx.set_flags(binding.WH_FLAG_PARITY_EXACT)
    with pytest.raises(binding.WhisperHipError, match="PARITY_EXACT"):
        ctx.set_constraint(*dfa.args, penalty=100.0)
    ctx.set_flags(0)
    ctx.set_constraint(*dfa.args, penalty=100.0)
    with pytest.raises(binding.WhisperHipError, match="constraint"):
        ctx.set_flags(binding.WH_FLAG_PARITY_EXACT)
    ctx.close()
    group = binding.HipContext(model, 1, hypotheses=2)
    with pytest.raises(binding.WhisperHipError, match="hypothesis-group"):
        group.set_constraint(*dfa.args, penalty=100.0)
    group.close()
