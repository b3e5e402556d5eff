"""What the decoding fallback costs the lock-step batch runner, on the device.

    python tools/batch_fallback_probe.py [--out profiles/batch_fallback_probe.json] [--launches 30] [--streams 64] [--skip-runner]

step    the sampler of one decode step at 64 and 448 rows of 51865 columns, every row greedy: the per-row step of wh_context_set_sampling_rows (table
        softmax with a factor per row + the draw kernel's greedy branch) next to the fused greedy sampler on the same rows in the same run -- what a round
        with one retrying row costs its greedy neighbours. wh_debug_probe kind 5: hip events around each launch, 5 warm-up launches, the median of
        --launches, the logits rotating through buffers that together exceed the last-level cache (512 MB).
runner  BatchRunner.run of --streams 30 s streams on the ggml-medium shape (the scripted model of bench.py's through_boundary: 51 samples per window),
        the feature off and on with thresholds that never fire, alternating, three runs each after a warm-up of both: the extra work is one no-speech
        gather per round and the host's scoring. The ratio of the medians is recorded.
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


def step(binding, launches):
    from whisper_amd import ggml_format as gf
    m = binding.HipModel.from_ggml(gf.synth_model("test-d128", seed=1))           # the probe needs a context for its stream only
    ctx = binding.HipContext(m, 1)
    out = {}
    for rows in (64, 448):
        fused, per_row = [], []
        for _ in range(3):                                                       # alternating, in one run
            fused.append(ctx.probe(5, 0, rows, COLS, 0, launches) * 1e3)
            per_row.append(ctx.probe(5, 1, rows, COLS, 0, launches) * 1e3)
        out[str(rows)] = dict(fused_greedy_us=[round(x, 2) for x in fused], per_row_all_greedy_us=[round(x, 2) for x in per_row],
                              ratio=round(float(np.median(per_row) / np.median(fused)), 3))
    ctx.close()
    m.close()
    return out


def runner(n_streams):
    from whisper_amd import api, ggml_format as gf
    hp = gf.hparams_for("medium")
    sp = gf.special_tokens(hp)
    script = [sp["beg"]] + [1000 + i for i in range(49)] + [sp["beg"] + 1500, sp["eot"]]
    model = gf.scripted_model(script, 3 if hp.is_multilingual else 1, kind="medium", seed=7)
    rng = np.random.default_rng(3)
    pcm = (0.1 * rng.standard_normal(16000 * 30 * 4)).astype(np.float32)
    streams = [(pcm, (i % 4) * 480000, 480000) for i in range(n_streams)]
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "scripted.bin")
        gf.write_model(path, model)
        del model
        m = api.Model(path)
        r = m.create_batch_runner(max_slots=n_streams, groups=1)

        def one(on):
            r.set_fallback(logprob_thold=-1e30, entropy_thold=-1.0, no_speech_thold=2.0) if on else r.set_fallback(None)
            hr, _, per = r.run(streams, flags=api.NO_CONTEXT, want_results=False)
            assert hr == 0 and all(p == 0 for p in per)
            if on:
                assert all(len(w) == 1 and w[0]["attempts"] == 1 for w in r.window_stats)
            return r.last_run_seconds * 1e3

        one(False), one(True)                                                    # warm-up: contexts, graph capture, the gather's buffer
        off, on = [], []
        for _ in range(3):
            off.append(one(False))
            on.append(one(True))
        r.close()
        m.close()
    return dict(streams=n_streams, model="ggml-medium shape, scripted (51 samples per window)", off_ms=[round(x, 2) for x in off], on_never_fires_ms=[round(x, 2) for x in on],
                ratio=round(float(np.median(on) / np.median(off)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--skip-runner", action="store_true")
    a = ap.parse_args()
    from whisper_amd import binding
    res = dict(cols=COLS, launches=a.launches, step=step(binding, a.launches))
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
