"""Top-k and nucleus sampling (DESIGN.md section 7 "Top-k and nucleus sampling"): what the kernel costs.

nucleusLogitsKernel alone at nVocab 51865, rows 1 and 448, for top_k = 50 alone, top_p = 0.9 alone and both, every row at T = 1 (wh_debug_probe kind 5 variant
11: hip events around every launch, the median of 30, the logits rotating over buffers that are filled anew before one comes round again -- the kernel narrows its
input, and a narrowed row is no work; at 448 rows the buffers exceed the last-level cache, at 1 row they are 13 MB and stay cached, so that figure is the latency
on a cached row), and -- in the same process -- softMaxSampleKernel on the same number of rows
(variant 0), the sampler the filter sits in front of. The probe's logits are uniform in [-6, 6) on a 16-bit grid: they crowd the first histogram level as real
logits do, and hold ties.

    python tools/nucleus_probe.py          # prints one JSON line and writes it to profiles/nucleus_probe.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
V, REPS = 51865, 30


def main():
    from whisper_amd import binding as B, ggml_format as gf
    hp = gf.hparams_for("test-d128-ml")
    model = B.HipModel.from_ggml(gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=4))
    ctx = B.HipContext(model, 1)
    res = {"nVocab": V, "kernel": [], "note": "medians of 30; hip events around each launch, rotating logits refilled before reuse: beyond the last-level cache at 448 rows, cached at 1 row"}
    for rows in (1, 448):
        sampler_us = ctx.probe(5, 0, rows, V, 0, REPS) * 1e3
        for k, p in ((50, 1.0), (0, 0.9), (50, 0.9)):
            us = ctx.probe(5, 11, rows, V, k + 2048 * round(100 * p), REPS) * 1e3
            res["kernel"].append({"rows": rows, "top_k": k, "top_p": p, "us": round(us, 2), "GBps": round(rows * V * 4 / us * 1e-3, 1), "softMaxSample_us": round(sampler_us, 2)})
    ctx.close()
    model.close()
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, "profiles", "nucleus_probe.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
