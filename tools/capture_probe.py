"""What live capture costs per chunk, and how long a piece waits for its text.

    python tools/capture_probe.py [--out profiles/capture_probe.json] [--calls 300] [--latency] [--kernel-stats kernel_stats.csv]
    python tools/capture_probe.py --kernels-only          # the appends alone, for a kernel-trace run of their own (rocprofv3 --kernel-trace --stats)

1. Per chunk, at 160, 1600 and 16000 samples of mono s16: the wall time of one wh_capture_append (whisper_amd/csrc/capture.hip: one upload of the chunk in
   its own format, one launch that converts it and gives the voice-activity features of the frames it completes, one download of those features; the call
   waits for the capture's own stream), next to the UNFUSED route on the same build: conversion on the host, the samples appended to a host buffer, and
   wh_vad_features_host on the frames the chunk completed (upload, the whole-buffer kernel, download). Medians of --calls calls after a warm-up; the chunks
   rotate through 64 different arrays and the buffer is emptied whenever 30 s are full, so no call repeats the one before. Pageable host memory on both
   sides, as a caller has it.
2. --kernel-stats: the kernel's own duration, read from the stats of a kernel-trace run of --kernels-only (a run of its own, no counters), merged in.
3. --latency: pause to text -- the wall time of run_full on a 3 s piece, which is what runCapture's worker does from the post to the job's end -- on the
   ggml-medium shape, with bench.py's single-stream model, which is scripted to transcribe 51 tokens and the end of text per window whatever the audio
   (the tokens of every run are recorded next to its time).
Prints one JSON line."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNKS = (160, 1600, 16000)
CAP = 30 * 16000 + 16000
ROTATE = 64


def speech_like(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-0.5, 0.5, n) * (0.002 + (np.sin(2 * np.pi * np.arange(n) / (16000 * 0.9)) > -0.3))).astype(np.float32)


def make_capture(binding, gf):
    m = binding.HipModel.from_ggml(gf.synth_model("test-d128", seed=1))
    ctx = binding.HipContext(m, 1)
    h = C.c_void_p()
    binding.check(binding.lib().wh_capture_create(ctx.handle, 1, 0, CAP, C.byref(h)))
    return m, ctx, h


def fused(binding, h, chunk, calls, warmup=50):
    L = binding.lib()
    src = [np.clip(np.round(speech_like(chunk, 10 + i) * 32768.0), -32768, 32767).astype(np.int16) for i in range(ROTATE)]
    feat = np.empty((chunk // 256 + 2, 3), np.float32)
    n_new = C.c_int64()
    pos, wall = 0, []
    binding.check(L.wh_capture_clear(h))
    for i in range(warmup + calls):
        if pos + chunk > 30 * 16000:
            binding.check(L.wh_capture_clear(h))
            pos = 0
        a = src[i % ROTATE]
        t0 = time.perf_counter()
        rc = L.wh_capture_append(h, a.ctypes.data_as(C.c_void_p), 1, chunk, feat.ctypes.data_as(C.c_void_p), len(feat), C.byref(n_new))
        t1 = time.perf_counter()
        binding.check(rc)
        pos += chunk
        if i >= warmup:
            wall.append(t1 - t0)
    return wall


def unfused(binding, chunk, calls, warmup=50):
    L = binding.lib()
    src = [np.clip(np.round(speech_like(chunk, 10 + i) * 32768.0), -32768, 32767).astype(np.int16) for i in range(ROTATE)]
    buf = np.zeros(CAP, np.float32)
    feat = np.empty((chunk // 256 + 2, 3), np.float32)
    pos, wall = 0, []
    for i in range(warmup + calls):
        if pos + chunk > 30 * 16000:
            pos = 0
        a = src[i % ROTATE]
        t0 = time.perf_counter()
        buf[pos:pos + chunk] = a.astype(np.float32) / np.float32(32768.0)
        first, last = pos // 256, (pos + chunk) // 256
        if last > first:
            span = buf[256 * first:256 * last]
            binding.check(L.wh_vad_features_host(span.ctypes.data_as(C.c_void_p), len(span), feat.ctypes.data_as(C.c_void_p)))
        t1 = time.perf_counter()
        pos += chunk
        if i >= warmup:
            wall.append(t1 - t0)
    return wall


def stats(wall):
    us = np.asarray(wall) * 1e6
    return dict(median_us=float(np.median(us)), p10_us=float(np.percentile(us, 10)), p90_us=float(np.percentile(us, 90)), calls=len(us))


def latency(api, gf, repeats=5):
    """bench.py's single-stream model: the ggml-medium shape scripted to transcribe 51 tokens and the end of text per window, whatever the audio"""
    hp = gf.hparams_for("medium")
    cap = 102
    positions, kept = gf.carry_over_script(hp, 7, 49, cap)
    path = os.path.join(tempfile.mkdtemp(prefix="capture_probe_"), "scripted.bin")
    gf.write_model(path, gf.scripted_model_at(positions, kind="medium", seed=7))
    m = api.Model(path)
    ctx = m.create_context()
    os.remove(path)
    pieces = [speech_like(48000, 100 + i) for i in range(repeats + 1)]
    out = []
    for i, p in enumerate(pieces):
        t0 = time.perf_counter()
        ctx.run_full(p, flags=api.NO_CONTEXT, n_max_text_ctx=cap)
        t1 = time.perf_counter()
        if i:           # the first run captures the decode graphs
            out.append(dict(ms=(t1 - t0) * 1e3, tokens=sum(len(s["tokens"]) for s in ctx.results())))
    ctx.close()
    m.close()
    return dict(model="ggml-medium shape, scripted to transcribe 51 tokens + the end of text per window (bench.py's single-stream model)", piece_samples=48000,
                runs=out, median_ms=float(np.median([r["ms"] for r in out])))


def kernel_stats(path):
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "captureAppendKernel" in row.get("Name", ""):
                return dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3,
                            source="rocprofv3 --kernel-trace --stats over --kernels-only: all three chunk sizes together")
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--latency", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default="")
    a = ap.parse_args()
    from whisper_amd import api, binding, ggml_format as gf
    if binding.device_count() < 1:
        raise SystemExit("capture_probe: no GPU")
    m, ctx, h = make_capture(binding, gf)
    if a.kernels_only:
        for chunk in CHUNKS:
            fused(binding, h, chunk, a.calls)
        binding.check(binding.lib().wh_capture_destroy(h))
        return
    res = dict(format="s16 mono", rotate=ROTATE, chunks={})
    # warm the clocks and the first-use tables of both routes
    fused(binding, h, 1600, 200)
    unfused(binding, 1600, 50)
    for chunk in CHUNKS:
        f, u = stats(fused(binding, h, chunk, a.calls)), stats(unfused(binding, chunk, a.calls))
        res["chunks"][str(chunk)] = dict(fused=f, unfused=u, fused_over_unfused=f["median_us"] / u["median_us"], audio_ms=chunk / 16.0)
    binding.check(binding.lib().wh_capture_destroy(h))
    ctx.close()
    m.close()
    res["fused_not_slower_at_1600"] = res["chunks"]["1600"]["fused"]["median_us"] <= res["chunks"]["1600"]["unfused"]["median_us"]
    if a.kernel_stats:
        res["kernel"] = kernel_stats(a.kernel_stats)
    if a.latency:
        res["pause_to_text"] = latency(api, gf)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
