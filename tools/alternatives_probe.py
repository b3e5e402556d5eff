"""Token alternatives (DESIGN.md section 7 "Token alternatives"): what the kernel costs.

  kernel   topLogprobsKernel alone at nVocab 51865, rows 1 / 40 / 448 x k 1 / 5 / 8 (wh_debug_probe kind 5 variant 9: hip events around every launch, the median
           of 30, the logits rotating over buffers that together exceed the last-level cache), with the achieved bytes per second of rows x nVocab x 4; its
           sorted-insertion form the same way (variant 10, which also holds that form's ids against the kernel's); and -- in the same process --
           softMaxSampleKernel on the same number of rows (variant 0).
  step     one decode step of 448 sequences on the d = 128 test model (test-d128-ml: the vocabulary is the real one, the layers are not, so the share of the
           step is an upper bound): a window of 1 + 64 steps with the setting at k = 5 and off, alternating, the host's clock around start .. finish, the median
           of 7, divided by 65.

    python tools/alternatives_probe.py          # prints one JSON line and writes it to profiles/alternatives_probe.json
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
V, REPS = 51865, 30


def main():
    import numpy as np
    import torch
    from whisper_amd import binding as B, ggml_format as gf
    res = {"nVocab": V, "kernel": [], "note": "medians; kernel: hip events around each launch, logits rotating beyond the last-level cache"}
    hp = gf.hparams_for("test-d128-ml")
    model = B.HipModel.from_ggml(gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=4))
    ctx1 = B.HipContext(model, 1)
    for rows in (1, 40, 448):
        sampler_us = ctx1.probe(5, 0, rows, V, 0, REPS) * 1e3
        for k in (1, 5, 8):
            us = ctx1.probe(5, 9, rows, V, k, REPS) * 1e3
            insert_us = ctx1.probe(5, 10, rows, V, k, REPS) * 1e3              # the form that lost; the probe also holds its ids against the kernel's
            res["kernel"].append({"rows": rows, "k": k, "us": round(us, 2), "GBps": round(rows * V * 4 / us * 1e-3, 1),
                                  "sorted_insertion_us": round(insert_us, 2), "softMaxSample_us": round(sampler_us, 2)})
    ctx1.close()
    batch, n_steps = 448, 64
    ctx = B.HipContext(model, batch)
    rng = np.random.default_rng(17)
    ctx.encode(torch.from_numpy(rng.uniform(-1, 1, (batch, 80, 3000)).astype(np.float32)).cuda())
    sp = gf.special_tokens(hp)
    prompt = np.array([[sp["prev"], 1000 + b % 64, sp["sot"], sp["sot"] + 1] for b in range(batch)], np.int32)
    times = {0: [], 5: []}
    for rep in range(8):
        for k in (0, 5):
            ctx.set_alternatives(k)
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.decode_window_start(prompt, n_steps)
            ctx.decode_window_finish()
            if rep:                                                              # the first round captures
                times[k].append((time.perf_counter() - t0) / (1 + n_steps) * 1e6)
    off, on = (sorted(times[k])[len(times[k]) // 2] for k in (0, 5))
    res["step"] = {"sequences": batch, "model": "test-d128-ml", "k": 5, "off_us": round(off, 1), "on_us": round(on, 1), "added_us": round(on - off, 1)}
    ctx.close()
    model.close()
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, "profiles", "alternatives_probe.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
