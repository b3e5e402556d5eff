"""Scoring a given transcript: the reduction kernel against the vocabulary softmax, and where the time of a whole wh_score_tokens call goes.

    python tools/score_probe.py [--out profiles/score_probe.json] [--launches 30] [--windows 64 --tokens 100]

1. tokenScoreKernel (wh_op_token_scores: one read of the row, 16 bytes written) at 1, 64 and 256 rows of 51865 logits against wh_op_vocab_soft_max ALONE on the
   same rows (one read, one write of the row). hip-event time per launch, warm-up first, median of --launches launches; the inputs rotate through buffers that
   together exceed the last-level cache (512 MB). wh_op_token_scores downloads and checks its targets before it launches, so the events around one call also
   bracket a device-to-host copy and a host wait (`score_op_us`; `check_overhead_us` is the same call on one row of 64 logits): that figure is the entry point's,
   not the kernel's. The kernels' own durations come from a kernel trace of this script, `rocprofv3 --kernel-trace --output-format csv -- python
   tools/score_probe.py --windows 0`, which `--trace-csv FILE` folds into the result: the median per kernel and row count (`kernel_us`, GB/s over the bytes the
   kernel moves, the share of the data sheet's HBM rate).
2. The whole wh_score_tokens on the ggml-medium shape (random weights) for --windows windows x --tokens scored tokens: wall time, and the per-class GPU time of
   wh_profile_read split into the teacher-forced pass, the vocabulary products (class gemmTiled: nothing else of the call uses it) and the reductions (class
   softMaxSample: the gather of the rows and tokenScoreKernel).
Prints one JSON line."""
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
HBM_GB_S = 8000.0           # the data sheet's rate of one MI355X, for the share a launch achieves


def ptr(t):
    return C.c_void_p(t.data_ptr())


def timed(torch, fn, bufs, launches, warmup=5):
    for i in range(warmup):
        fn(bufs[i % len(bufs)])
    torch.cuda.synchronize()
    ms = []
    for i in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(bufs[(warmup + i) % len(bufs)])
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)) * 1e3


def kernel_alone(torch, binding, launches):
    L = binding.lib()
    tiny = torch.randn((1, 64), device="cuda", dtype=torch.float32)
    tiny_t = torch.zeros((1,), dtype=torch.int32, device="cuda")
    tiny_o = torch.empty((4,), dtype=torch.int32, device="cuda")
    overhead = timed(torch, lambda x: binding.op_token_scores(ptr(x), 64, 1, 64, ptr(tiny_t), ptr(tiny_o)), [tiny], launches)
    out = dict(check_overhead_us=overhead, rows={})
    for rows in (1, 64, 256):
        row_bytes = rows * COLS * 4
        n_buf = min(ROTATE_BYTES // row_bytes + 2, 64)          # (one row: 64 buffers of 207 KB would all sit in the cache anyway; said in DESIGN.md)
        g = torch.Generator(device="cuda").manual_seed(rows)
        bufs = [3.0 * torch.randn((rows, COLS), generator=g, device="cuda", dtype=torch.float32) for _ in range(n_buf)]
        probs = torch.empty((rows, COLS), dtype=torch.float32, device="cuda")
        targets = torch.randint(0, COLS, (rows,), generator=g, device="cuda", dtype=torch.int32)
        recs = torch.empty((rows * 4,), dtype=torch.int32, device="cuda")
        score = timed(torch, lambda x: binding.op_token_scores(ptr(x), COLS, rows, COLS, ptr(targets), ptr(recs)), bufs, launches)
        soft = timed(torch, lambda x: binding.check(L.wh_op_vocab_soft_max(None, ptr(x), ptr(probs), rows, COLS)), bufs, launches)
        out["rows"][str(rows)] = dict(buffers=n_buf, score_op_us=score, soft_max_only_us=soft, soft_max_gb_s=2 * row_bytes / soft * 1e-3)
        del bufs
        torch.cuda.empty_cache()
    return out


def trace_summary(path):
    """A rocprofv3 kernel trace (CSV) of this script: per kernel of interest and row count (grid / 1024 threads) the median duration of its launches at 51865
    columns is not in the trace, so the row counts of kernel_alone -- 1, 64, 256 -- are taken; 1-row launches include the calibration call."""
    import csv
    by = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            kind = "score" if "tokenScoreKernel" in name else "soft_max" if "softMaxRowsReg" in name else None
            if kind is None:
                continue
            rows = int(r["Grid_Size_X"]) // 1024 if int(r["Grid_Size_X"]) >= 1024 else int(r["Grid_Size_X"])
            by.setdefault((kind, rows), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    out = {}
    for (kind, rows), us in sorted(by.items()):
        if rows not in (1, 64, 256):
            continue
        # the one-row calibration launches (64 columns) are the shortest of the one-row launches: the upper half is the 51865-column row
        us = sorted(us)
        if kind == "score" and rows == 1:
            us = us[len(us) // 2:]
        med = float(np.median(us))
        moved = rows * COLS * 4 * (2 if kind == "soft_max" else 1)
        out.setdefault(str(rows), {})[kind] = dict(launches=len(us), kernel_us=med, gb_s=moved / med * 1e-3, hbm_share=moved / med * 1e-3 / HBM_GB_S)
    return out


def whole_call(torch, binding, windows, tokens, repeats=5):
    import bench
    from whisper_amd import ggml_format as gf
    model = gf.synth_model("medium", seed=1)
    sp = gf.special_tokens(model.hparams)
    m = binding.HipModel.from_ggml(model)
    del model
    ctx = binding.HipContext(m, windows)
    pcm = torch.from_numpy(bench.synth_pcm(7, seed=100)).cuda()
    mels = ctx.mel_spectrogram_batch(pcm)
    ctx.encode_windows([(mels[i % 7], 0) for i in range(windows)])
    rng = np.random.default_rng(5)
    head = [sp["sot"], sp["sot"] + 1, sp["transcribe"], sp["not_"]]
    rows = [head + [int(t) for t in rng.integers(0, sp["eot"], tokens - 1)] + [sp["eot"]] for _ in range(windows)]
    lens, firsts = [len(r) for r in rows], [len(head)] * windows

    def call():
        ctx.score_tokens(rows, lens, firsts)

    call()
    wall = []
    for _ in range(repeats):
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        wall.append(time.perf_counter() - t0)
    ctx.profile(True)
    call()
    prof = ctx.profile_read()
    ctx.profile(False)
    ms = {k: v["ms"] for k, v in prof.items() if v["calls"] and k != "eventPair"}
    products, reductions = ms.get("gemmTiled", 0.0), ms.get("softMaxSample", 0.0)
    out = dict(windows=windows, scored_tokens=tokens, rows_per_window=len(rows[0]), scored_rows=windows * tokens, chunk_rows=binding.get_option("score_chunk_rows"),
               wall_ms=float(np.median(wall)) * 1e3, profiled_ms=ms, pass_ms=sum(ms.values()) - products - reductions, products_ms=products, reductions_ms=reductions,
               product_calls=prof.get("gemmTiled", {}).get("calls", 0))
    ctx.close()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--tokens", type=int, default=100)
    ap.add_argument("--trace-csv", default="", help="a rocprofv3 kernel trace of this script: only fold its per-kernel medians into --out (no device needed)")
    a = ap.parse_args()
    if a.trace_csv:
        res = {}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.loads(f.read())
        res["kernel_trace"] = trace_summary(a.trace_csv)
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    import torch
    from whisper_amd import binding
    res = dict(cols=COLS, launches=a.launches, kernel=kernel_alone(torch, binding, a.launches))
    if a.windows > 0:
        res["call"] = whole_call(torch, binding, a.windows, a.tokens)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
