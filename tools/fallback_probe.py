"""The decoding fallback's two kernels and the cost of one more attempt, on the device.

    python tools/fallback_probe.py [--out profiles/fallback_probe.json] [--launches 30] [--steps 100]

wh_op_vocab_soft_max_scaled and wh_op_sample_draw at 1 and 64 rows of 51865 columns, next to wh_op_vocab_soft_max and wh_op_sample_best on the same rows:
hip-event time per launch, warm-up first, median of --launches launches. The logits rotate through buffers that together exceed the last-level cache
(512 MB); the draw and the greedy sampler read the probabilities the softmax before them just wrote, as they do in a decode step. Then the wall time of
one attempt of a window on the single-stream path (ggml-medium shape, random weights, one sequence): the prompt step and --steps device-side steps,
greedy and at temperature 0.6, the encoder's output left where it is -- what a further attempt of the fallback costs. Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLS = 51865
ROTATE_BYTES = 512 << 20


def ptr(t):
    return C.c_void_p(t.data_ptr())


def timed(torch, fn, bufs, launches, before=None, warmup=5):
    for i in range(warmup):
        if before:
            before(bufs[i % len(bufs)])
        fn(bufs[i % len(bufs)])
    torch.cuda.synchronize()
    ms = []
    for i in range(launches):
        x = bufs[(warmup + i) % len(bufs)]
        if before:
            before(x)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(x)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)) * 1e3


def attempt(torch, binding, steps, repeats=7):
    from whisper_amd import ggml_format as gf
    model = gf.synth_model("medium", seed=1)
    sp = gf.special_tokens(model.hparams)
    m = binding.HipModel.from_ggml(model)
    del model
    ctx = binding.HipContext(m, 1)
    rng = np.random.default_rng(5)
    ctx.encode(torch.from_numpy(rng.uniform(-1, 1, (1, 80, 3000)).astype(np.float32)).cuda())
    prompt = np.asarray([[sp["sot"], sp["sot"] + 1, sp["transcribe"]]], np.int32)

    def wall():
        t = []
        for i in range(repeats + 2):                       # the first window of a mode captures its step graph
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.decode_window_start(prompt, steps)
            ctx.decode_window_finish()
            t.append(time.perf_counter() - t0)
        return float(np.median(t[2:])) * 1e3, t[0] * 1e3

    out = dict(model="medium shape, random weights", sequences=1, steps=steps)
    out["greedy_attempt_ms"], out["greedy_first_window_ms"] = wall()
    ctx.set_sampling(0.6, 1, 1)
    out["sampled_attempt_ms"], out["sampled_first_window_ms"] = wall()
    ctx.set_sampling(0.0)
    out["greedy_again_first_window_ms"] = wall()[1]
    ctx.close()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--steps", type=int, default=100)
    a = ap.parse_args()
    import torch
    from types import SimpleNamespace
    from whisper_amd import binding, ggml_format as gf
    L = binding.lib()
    sp = gf.special_tokens(SimpleNamespace(n_vocab=COLS))
    ids = (sp["beg"], sp["sot"], sp["solm"], sp["not_"])
    res = dict(cols=COLS, launches=a.launches, rows={})
    for rows in (1, 64):
        n_buf = min(64, ROTATE_BYTES // (rows * COLS * 4) + 2)
        g = torch.Generator(device="cuda").manual_seed(rows)
        bufs = [3.0 * torch.randn((rows, COLS), generator=g, device="cuda", dtype=torch.float32) for _ in range(n_buf)]
        probs = torch.empty((rows, COLS), dtype=torch.float32, device="cuda")
        pos = torch.arange(rows, dtype=torch.int32, device="cuda")
        out = torch.zeros(rows * 5, dtype=torch.int32, device="cuda")

        def soft_max(x):
            binding.check(L.wh_op_vocab_soft_max(None, ptr(x), ptr(probs), rows, COLS))

        def scaled(x):
            binding.check(L.wh_op_vocab_soft_max_scaled(None, ptr(x), 1.25, ptr(probs), rows, COLS))

        def best(x):
            binding.check(L.wh_op_sample_best(None, ptr(probs), rows, COLS, *ids, 0, 0, ptr(out)))

        def draw(x):
            binding.check(L.wh_op_sample_draw(None, ptr(probs), rows, COLS, *ids, 0, 0, 7, 3, ptr(pos), ptr(out)))

        res["rows"][str(rows)] = dict(buffers=n_buf, soft_max_us=timed(torch, soft_max, bufs, a.launches), soft_max_scaled_us=timed(torch, scaled, bufs, a.launches),
                                      sample_best_us=timed(torch, best, bufs, a.launches, before=scaled), sample_draw_us=timed(torch, draw, bufs, a.launches, before=scaled))
        del bufs
        torch.cuda.empty_cache()
    res["attempt"] = attempt(torch, binding, a.steps)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
