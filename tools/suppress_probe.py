"""What suppressed tokens cost, on the device.

    python tools/suppress_probe.py [--out profiles/suppress_probe.json] [--launches 30] [--streams 64] [--skip-runner]

kernel  the logit filter alone (suppressLogitsKernel: one workgroup per row, -inf at the set's columns) at 1, 64 and 448 rows of 51865 columns with 88 and 4096
        ids. wh_debug_probe kind 5 variant 3: hip events around each launch, 5 warm-up launches, the median of --launches, the logits rotating through buffers
        that together exceed the last-level cache (512 MB; at most 64 buffers, which a single row does not reach).
step    the sampler of one decode step at 64 and 448 rows, the fused greedy sampler alone (variant 0) and behind the filter with 88 ids (variant 2),
        alternating three times in one run.
runner  BatchRunner.run of --streams 30 s streams on the ggml-medium shape (the scripted model of bench.py's through_boundary: 51 samples per window), the set
        off and on with the model's non-speech set, alternating, three runs each after a warm-up of both. The ratio of the medians is recorded.
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


def spread(xs):
    return round(float(max(xs) - min(xs)), 2)


def kernel_and_step(binding, launches):
    from whisper_amd import ggml_format as gf
    m = binding.HipModel.from_ggml(gf.synth_model("test-d128", seed=1))           # the probe needs a context for its stream only
    ctx = binding.HipContext(m, 1)
    kernel, step = {}, {}
    for rows in (1, 64, 448):
        for n_ids in (88, 4096):
            us = [ctx.probe(5, 3, rows, COLS, n_ids, launches) * 1e3 for _ in range(3)]
            kernel["%dx%d" % (rows, n_ids)] = dict(us=[round(x, 2) for x in us], median_us=round(float(np.median(us)), 2))
    for rows in (64, 448):
        off, on = [], []
        for _ in range(3):                                                       # alternating, in one run
            off.append(ctx.probe(5, 0, rows, COLS, 0, launches) * 1e3)
            on.append(ctx.probe(5, 2, rows, COLS, 88, launches) * 1e3)
        step[str(rows)] = dict(fused_greedy_us=[round(x, 2) for x in off], filter_88_and_fused_greedy_us=[round(x, 2) for x in on], spread_off_us=spread(off),
                               spread_on_us=spread(on), extra_us=round(float(np.median(on) - np.median(off)), 2), ratio=round(float(np.median(on) / np.median(off)), 3))
    ctx.close()
    m.close()
    return kernel, step


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
        ids = m.non_speech_tokens()
        r = m.create_batch_runner(max_slots=n_streams, groups=1)

        def one(on):
            r.set_suppress_tokens(ids if on else None)
            hr, _, per = r.run(streams, flags=api.NO_CONTEXT, want_results=False)
            assert hr == 0 and all(p == 0 for p in per)
            return r.last_run_seconds * 1e3

        one(False), one(True)                                                    # warm-up: contexts, both graph captures, the set's buffer
        off, on = [], []
        for _ in range(3):
            off.append(one(False))
            on.append(one(True))
        r.close()
        m.close()
    return dict(streams=n_streams, model="ggml-medium shape, scripted (51 samples per window)", ids=len(ids), off_ms=[round(x, 2) for x in off],
                on_non_speech_ms=[round(x, 2) for x in on], spread_off_ms=spread(off), spread_on_ms=spread(on), ratio=round(float(np.median(on) / np.median(off)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--skip-runner", action="store_true")
    a = ap.parse_args()
    from whisper_amd import binding
    kernel, step = kernel_and_step(binding, a.launches)
    res = dict(cols=COLS, launches=a.launches, mapping="one workgroup of 256 threads per row", kernel=kernel, step=step)
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
