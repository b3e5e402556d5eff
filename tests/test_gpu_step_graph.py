"""GPU tests of the owner of captured decode steps (csrc/step_graph.hip; DESIGN.md section 7, "Decode step = one captured hipGraph"): its key, its retention rule
and its two warm-up protocols. Every comparison is between a context that replays graphs and one that launches the same kernels eagerly (WH_FLAG_NO_GRAPH) or
enqueues them in one piece, so token ids and every float are compared by their bits. The capture counts are stated from the retention rule:

  * a greedy step is captured when no graph of its (batch, key) is held; capturing it destroys the greedy graphs of another batch or of a key that differs in
    anything but the per-row bit -- so the flip of a mode captures once, and the per-row sibling survives leaving and re-entering its mode;
  * there is at most one beam graph, replaced when its batch, width or key (the parity mode, "a suppressed set is held") differs;
  * neither kind ever destroys the other's."""
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from whisper_amd import binding, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("id", "tid", "p", "pt", "ptsum")
BEAM_FIELDS = FIELDS + ("parent", "finished")


@pytest.fixture(scope="module")
def random_weights():
    """The random-weight model of the suppress tests: a weight scale at which text tokens and timestamps are both sampled"""
    hp = gf.hparams_for("test-d128")
    model = binding.HipModel.from_ggml(gf.synth_model("test-d128", seed=31, w_std=0.3))
    yield SimpleNamespace(hp=hp, model=model, sp=gf.special_tokens(hp))
    model.close()


def _mels(batch):
    rng = np.random.default_rng(17)
    return torch.from_numpy(rng.uniform(-1, 1, (batch, 80, 3000)).astype(np.float32)).cuda()


def _context(c, batch, flags=0, hypotheses=1):
    ctx = binding.HipContext(c.model, batch, hypotheses=hypotheses)
    ctx.set_flags(flags)
    ctx.encode(_mels(batch))
    return ctx


def _prompts(sp, batch, n=3):
    return np.array([[sp["sot"], 1000 + 13 * b, 2000 + 7 * b, sp["not_"]][:n] for b in range(batch)], np.int32)


def _window(ctx, prompt, n_steps):
    ctx.decode_window_start(prompt, n_steps)
    data = ctx.decode_window_fetch_data(0, 1 + n_steps)
    ctx.decode_window_finish()
    return data


def _same(a, b, fields=FIELDS):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)) for k in fields)


@pytest.mark.parametrize("batch", [3, 5])
def test_mode_walk_on_one_context(random_weights, batch):
    """One context walks through the modes that are bits of the key, a window of 8 steps in each, at 3 rows (the single-stream step) and 5 (the batched one).
    Every window equals the same window of a WH_FLAG_NO_GRAPH context put through the same calls, and the capture counter follows the retention rule."""
    c, sp = random_weights, random_weights.sp
    prompt = _prompts(sp, batch)
    graph, eager = _context(c, batch), _context(c, batch, binding.WH_FLAG_NO_GRAPH)
    temps = [0.0] * batch
    temps[1] = 0.9
    rows_on = lambda x: x.set_sampling_rows(temps, [77 + b for b in range(batch)], [5] * batch)
    rows_off = lambda x: x.set_sampling_rows(None)
    suppressed = [5, 1000, 1013, 2000, 2007, sp["eot"] - 1]
    walk = [
        # what happens                     expected captures so far, by the rule
        ("greedy", lambda x: None, 1),                                           # nothing is held
        ("suppress on", lambda x: x.set_suppress(suppressed), 2),                # a flip: one capture, the graph without the filter goes
        ("rules on", lambda x: x.set_timestamp_rules(True), 3),                  # a flip
        ("per-row on", rows_on, 4),                                              # entering the per-row mode: one capture, the sibling stays
        ("per-row off", rows_off, 4),                                            # the sibling is still there
        ("rules off", lambda x: x.set_timestamp_rules(False), 5),                # a flip: both graphs with the rules go
        ("suppress off", lambda x: x.set_suppress(None), 6),                     # a flip
        # ... and behind the walk: leaving the per-row mode and entering it again captures nothing
        ("per-row on again", rows_on, 7),
        ("per-row off again", rows_off, 7),
        ("per-row on a third time", rows_on, 7),
    ]
    seen = []
    for name, change, captures in walk:
        change(graph)
        change(eager)
        a, b = _window(graph, prompt, 8), _window(eager, prompt, 8)
        assert _same(a, b), name
        assert graph.step_captures() == captures, (name, graph.step_captures(), captures)
        seen.append(a["id"].copy())
    assert eager.step_captures() == 0
    # the modes are real: the filter, the rules and the tempered row each change what is decoded
    assert not np.array_equal(seen[0], seen[1]) or not np.array_equal(seen[1], seen[2]) or not np.array_equal(seen[2], seen[3])
    assert np.array_equal(seen[0], seen[6])
    graph.close()
    eager.close()


@pytest.mark.parametrize("batch", [3, 5])
def test_capture_inside_continue_preserves_the_window(random_weights, batch):
    """WARM_PRESERVE under wh_decode_window_continue: a ragged window (prompts of 2 and 4 tokens, the timestamp rules on) started WITHOUT steps captures nothing;
    the 6 steps of the continue capture over the window's live state -- sampler state, ragged positions, pending tokens, timestamp records. The samples equal
    those of a fresh context that enqueues the window in one piece."""
    c, sp = random_weights, random_weights.sp
    prompts = [list(_prompts(sp, batch, 4)[b][:(2, 4)[b % 2]]) for b in range(batch)]
    runs = []
    for split in (True, False):
        ctx = _context(c, batch)
        ctx.set_timestamp_rules(True)
        ctx.decode_window_start_ragged(prompts, 0 if split else 6)
        if split:
            assert ctx.step_captures() == 0
            ctx.decode_window_continue(6)
        assert ctx.step_captures() == 1
        runs.append(ctx.decode_window_fetch_data(0, 7))
        ctx.decode_window_finish()
        ctx.close()
    assert _same(runs[0], runs[1])


@pytest.mark.parametrize("batch", [3, 5])
def test_first_greedy_call_behind_a_prompt_preserves_the_cache(random_weights, batch):
    """WARM_PRESERVE under wh_decode_greedy: a wh_decode prompt of 3 tokens fills cache rows 0 .. 2, then the first wh_decode_greedy of a fresh context (nPast = 3)
    captures. A warm-up at position 0 would overwrite row 0 of the live cache; the 6 samples equal those of a WH_FLAG_NO_GRAPH context. A second round on the
    same context captures nothing and gives the same."""
    c, sp = random_weights, random_weights.sp
    prompt = _prompts(sp, batch)
    first = np.array([3000 + 11 * b for b in range(batch)], np.int32)

    def run(ctx):
        ctx.decode(prompt, 0, want_logits=False, want_probs=False)
        _, data = ctx.decode_greedy(first, prompt.shape[1], 6)
        return {k: np.array([[d[k] for d in step] for step in data], np.int32 if k in ("id", "tid") else np.float32) for k in FIELDS}

    graph, eager = _context(c, batch), _context(c, batch, binding.WH_FLAG_NO_GRAPH)
    want = run(eager)
    assert _same(run(graph), want) and graph.step_captures() == 1
    assert _same(run(graph), want) and graph.step_captures() == 1
    graph.close()
    eager.close()


def _beam_window(ctx, prompt, width, n_steps):
    ctx.beam_window_start(prompt, width, n_steps)
    return ctx.beam_window_status(), ctx.beam_window_records(0, 1 + n_steps)


def test_beam_step_is_keyed_like_the_greedy_step(random_weights):
    """2 windows x 3 hypotheses, width 3, 6 forced steps. The parity mode is part of the beam step's key: a window under flags 0, one under WH_FLAG_PARITY_PV with 2
    threads and one under flags 0 again each capture once, and each equals the window of a WH_FLAG_NO_GRAPH context under the same flags (records and search
    states). A greedy window between two beam windows of one shape destroys nothing: the second beam window captures nothing, nor does the next greedy one.

    On the commit before the beam step had a key, the second window replayed the step captured under flags 0: run there, that window had the eager context's ids
    and parents but 36 of 42 records with other p / pt / ptsum bits (up to 2.55e-3 apart) and another search state; the first and third window were equal."""
    c, sp = random_weights, random_weights.sp
    windows, hyp, width, n_steps = 2, 3, 3, 6
    prompt = _prompts(sp, windows)
    graph, eager = _context(c, windows, 0, hyp), _context(c, windows, binding.WH_FLAG_NO_GRAPH, hyp)
    results = []
    for captures, (flags, threads) in enumerate([(0, 1), (binding.WH_FLAG_PARITY_PV, 2), (0, 1)], 1):
        graph.set_flags(flags, threads)
        eager.set_flags(flags | binding.WH_FLAG_NO_GRAPH, threads)
        for x in (graph, eager):
            x.encode(_mels(windows))
        (st_a, rec_a), (st_b, rec_b) = _beam_window(graph, prompt, width, n_steps), _beam_window(eager, prompt, width, n_steps)
        assert _same(rec_a, rec_b, BEAM_FIELDS) and st_a == st_b, (flags, threads)
        assert graph.step_captures() == captures, (flags, threads, graph.step_captures())
        results.append((st_a, rec_a))
    assert _same(results[0][1], results[2][1], BEAM_FIELDS) and results[0][0] == results[2][0]
    # the two kinds of step live side by side
    greedy_prompt = _prompts(sp, windows * hyp)
    g_a, g_b = _window(graph, greedy_prompt, 8), _window(eager, greedy_prompt, 8)
    assert _same(g_a, g_b) and graph.step_captures() == 4
    st, rec = _beam_window(graph, prompt, width, n_steps)
    assert graph.step_captures() == 4
    assert _same(rec, results[2][1], BEAM_FIELDS) and st == results[2][0]
    assert _same(_window(graph, greedy_prompt, 8), g_a) and graph.step_captures() == 4
    assert eager.step_captures() == 0
    graph.close()
    eager.close()
