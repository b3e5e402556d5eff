"""What phrase boosting costs, on the device.

    python tools/phrase_boost_probe.py [--out profiles/phrase_boost_probe.json] [--launches 30] [--streams 64] [--skip-runner]

kernel  the filter alone (boostLogitsKernel: one workgroup of 256 threads per row, an automaton state per row, the boost added to the offered columns) at 1, 64
        and 448 rows of 51865 columns for three sets: one phrase, 64 phrases, 1024 phrases with 1024 distinct first tokens (two tokens each). Every row has
        just sampled the first token of a phrase, so the launch searches the fed token in the node's table, boosts the node's offer and holds every root token
        against the node's table. wh_debug_probe kind 5 variant 6: hip events around each launch, 5 warm-up launches, the median of --launches, the logits
        rotating through buffers that together exceed the last-level cache (512 MB; at most 64 buffers, which a single row does not reach).
        Beside it, in the same session, the timestamp-rules filter alone (variant 5) for its three histories: the comparator, a kernel that sweeps whole rows.
runner  BatchRunner.run of --streams 30 s streams on the ggml-medium shape (the scripted model of bench.py's through_boundary: 51 samples per window), the set
        off and on, alternating, three timed runs each after a warm-up of both. Turning the set on or off changes the captured step's key and drops the other
        side's graph, so on each side an untimed run goes first (it recaptures) and the run behind it is timed. The set is 47 three-token phrases of the script's own text and a boost of 2 -- below
        the margin the scripted tokens win by, so both sides decode the same transcript and differ in the filter's launches only. The ratio of the medians is
        recorded.
Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLS = 51865
SETS = (("1_phrase", 0), ("64_phrases", 1), ("1024_first_tokens", 2))
HISTORIES = (("text", 0), ("closed", 1), ("open", 2))


def spread(xs):
    return round(float(max(xs) - min(xs)), 2)


def kernels(binding, launches):
    from whisper_amd import ggml_format as gf
    m = binding.HipModel.from_ggml(gf.synth_model("test-d128", seed=1))           # the probe needs a context for its stream only
    ctx = binding.HipContext(m, 1)
    boost, rules = {}, {}
    for rows in (1, 64, 448):
        for (name, k), (hist, kh) in zip(SETS, HISTORIES):                       # alternating the two filters, in one run
            us = [ctx.probe(5, 6, rows, COLS, k, launches) * 1e3 for _ in range(3)]
            boost["%dx%s" % (rows, name)] = dict(us=[round(x, 2) for x in us], median_us=round(float(np.median(us)), 2), spread_us=spread(us))
            us = [ctx.probe(5, 5, rows, COLS, kh, launches) * 1e3 for _ in range(3)]
            rules["%dx%s" % (rows, hist)] = dict(us=[round(x, 2) for x in us], median_us=round(float(np.median(us)), 2), spread_us=spread(us))
    ctx.close()
    m.close()
    return boost, rules


def runner(n_streams):
    from whisper_amd import api, ggml_format as gf
    hp = gf.hparams_for("medium")
    sp = gf.special_tokens(hp)
    script = [sp["beg"]] + [1000 + i for i in range(49)] + [sp["beg"] + 1500, sp["eot"]]
    model = gf.scripted_model(script, 3 if hp.is_multilingual else 1, kind="medium", seed=7)
    rng = np.random.default_rng(3)
    pcm = (0.1 * rng.standard_normal(16000 * 30 * 4)).astype(np.float32)
    streams = [(pcm, (i % 4) * 480000, 480000) for i in range(n_streams)]
    phrases = [[1000 + i, 1001 + i, 1002 + i] for i in range(47)]
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "scripted.bin")
        gf.write_model(path, model)
        del model
        m = api.Model(path)
        r = m.create_batch_runner(max_slots=n_streams, groups=1)

        def setting(on):
            r.set_boost_phrases(phrases if on else None, 2.0 if on else None)

        def one(on):
            # a change of the setting changes the step graph's key and the other side's graph is dropped: the first run behind it pays a warm-up step and a
            # capture, the second replays. The second is the one timed
            setting(on)
            for _ in range(2):
                hr, _, per = r.run(streams, flags=api.NO_CONTEXT, want_results=False)
                assert hr == 0 and all(p == 0 for p in per)
            return r.last_run_seconds * 1e3

        def transcript(on):
            setting(on)
            hr, res, _ = r.run(streams[:1], flags=api.NO_CONTEXT)
            assert hr == 0
            return [t["id"] for s in res[0] for t in s["tokens"]]

        plain = transcript(False)
        assert transcript(True) == plain and len(plain) >= 49, "the set must not change the scripted transcript"
        one(False), one(True)                                                    # warm-up: contexts, the tables
        off, on = [], []
        for _ in range(3):
            off.append(one(False))
            on.append(one(True))
        r.close()
        m.close()
    return dict(streams=n_streams, model="ggml-medium shape, scripted (51 samples per window)", phrases=len(phrases), boost=2.0, same_transcript=True,
                off_ms=[round(x, 2) for x in off], on_ms=[round(x, 2) for x in on], spread_off_ms=spread(off), spread_on_ms=spread(on),
                ratio=round(float(np.median(on) / np.median(off)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--skip-runner", action="store_true")
    a = ap.parse_args()
    from whisper_amd import binding
    boost, rules = kernels(binding, a.launches)
    res = dict(cols=COLS, launches=a.launches, mapping="one workgroup of 256 threads per row", boost_filter=boost, timestamp_rules_filter=rules)
    if not a.skip_runner:
        res["runner"] = runner(a.streams)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
