"""What no-repeat n-grams cost, on the device.

    python tools/no_repeat_probe.py [--out profiles/no_repeat_probe.json] [--launches 30] [--skip-loop]

kernel  the filter alone (noRepeatKernel: one workgroup of 256 threads per row, a history of up to 448 tokens per row, one -inf per start position whose
        n - 1 tokens equal the last n - 1) at 64 and 448 rows of 51865 columns, n = 3, for histories of 8 and of 440 tokens of a five-letter alphabet, so every
        start position's n-gram recurs and stores. wh_debug_probe kind 5 variant 8: hip events around each launch, 5 warm-up launches, the median of --launches,
        the logits rotating through buffers that together exceed the last-level cache (512 MB; at most 64 buffers).
step    the sampler of one decode step at the same shapes: the fused greedy sampler alone (variant 0 -- the step as it is without the filter) and behind the
        filter (variant 7) for each history, alternating three times in one run.
loop    the device-side loop itself: wh_decode_window_start of 200 steps on the synthetic test-d128-ml model at 1, 5 and 64 rows, the option off and on
        (n = 3), alternating, three windows each after a warm-up of both (graph captures, the histories' allocation); wall time per step.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLS = 51865
ROWS = (64, 448)
HISTORIES = (8, 440)
N = 3                                                                            # what wh_debug_probe's variants 7 and 8 run


def spread(xs):
    return round(float(max(xs) - min(xs)), 2)


def kernel_and_step(binding, launches):
    from whisper_amd import ggml_format as gf
    m = binding.HipModel.from_ggml(gf.synth_model("test-d128", seed=1))           # the probe needs a context for its stream only
    ctx = binding.HipContext(m, 1)
    kernel, step = {}, {}
    for rows in ROWS:
        for k in HISTORIES:
            us = [ctx.probe(5, 8, rows, COLS, k, launches) * 1e3 for _ in range(3)]
            kernel["%dxh%d" % (rows, k)] = dict(us=[round(x, 2) for x in us], median_us=round(float(np.median(us)), 2))
    for rows in ROWS:
        for k in HISTORIES:
            off, on = [], []
            for _ in range(3):                                                   # alternating, in one run
                off.append(ctx.probe(5, 0, rows, COLS, 0, launches) * 1e3)
                on.append(ctx.probe(5, 7, rows, COLS, k, launches) * 1e3)
            step["%dxh%d" % (rows, k)] = dict(fused_greedy_us=[round(x, 2) for x in off], filter_and_fused_greedy_us=[round(x, 2) for x in on],
                                              spread_off_us=spread(off), spread_on_us=spread(on), extra_us=round(float(np.median(on) - np.median(off)), 2),
                                              ratio=round(float(np.median(on) / np.median(off)), 3))
    ctx.close()
    m.close()
    return kernel, step


def loop(binding, n_steps=200):
    import torch
    from whisper_amd import ggml_format as gf
    model = gf.synth_model("test-d128-ml", seed=31)
    sp = gf.special_tokens(model.hparams)
    m = binding.HipModel.from_ggml(model)
    out = {}
    for rows in (1, 5, 64):
        ctx = binding.HipContext(m, rows)
        rng = np.random.default_rng(17)
        ctx.encode(torch.from_numpy(rng.uniform(-1, 1, (rows, 80, 3000)).astype(np.float32)).cuda())
        prompt = np.array([[sp["sot"], sp["sot"] + 1, sp["transcribe"]]] * rows, np.int32)

        def one(n):
            ctx.set_no_repeat(n)
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.decode_window_start(prompt, n_steps)
            ctx.decode_window_finish()
            return (time.perf_counter() - t0) * 1e6 / (1 + n_steps)

        one(0), one(N)
        off, on = [], []
        for _ in range(3):
            off.append(one(0))
            on.append(one(N))
        ctx.set_no_repeat(0)
        ctx.close()
        out[str(rows)] = dict(steps=n_steps, off_us_per_step=[round(x, 2) for x in off], on_us_per_step=[round(x, 2) for x in on], spread_off_us=spread(off),
                              spread_on_us=spread(on), extra_us=round(float(np.median(on) - np.median(off)), 2), ratio=round(float(np.median(on) / np.median(off)), 4))
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--skip-loop", action="store_true")
    a = ap.parse_args()
    if not a.skip_loop:
        import torch
        torch.zeros(1).cuda()                                                    # torch takes the device first: the loop hands it torch tensors
    from whisper_amd import binding
    kernel, step = kernel_and_step(binding, a.launches)
    res = dict(cols=COLS, launches=a.launches, n=N, mapping="one workgroup of 256 threads per row", kernel=kernel, step=step)
    if not a.skip_loop:
        res["loop"] = loop(binding)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
