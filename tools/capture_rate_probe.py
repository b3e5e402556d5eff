"""What a chunk of live capture costs when the stream is not at 16 kHz and the chunk's launch resamples it.

    python tools/capture_rate_probe.py [--out profiles/capture_rate_probe.json] [--calls 300] [--kernel-stats kernel_stats.csv]
    python tools/capture_rate_probe.py --kernels-only     # the appends alone, for a kernel-trace run of their own (rocprofv3 --kernel-trace --stats)
    python tools/capture_rate_probe.py --merge-into profiles/capture_rate_probe.json --kernel-trace kernel_trace.csv --trace-calls 100      # no GPU

Per chunk of 10 ms, 100 ms and 1 s of audio, for 48 kHz s16 mono and for 44.1 kHz f32 stereo with the stereo kept: the wall time of one wh_capture_append on a
capture made by wh_capture_create_rate (whisper_amd/csrc/capture.hip: one upload of the chunk in its own format, one launch that resamples it -- three
filtered channels when the stereo of a two-channel source is kept --, appends the outputs that became ready and gives the voice-activity features of the frames
they complete, one download of those features; the call waits for the capture's own stream). Beside each: the 16 kHz append of the same audio duration, same
format and channels, on a capture made by wh_capture_create, measured in the same session right behind it, and the ratio of the medians. Medians and p10 / p90
of --calls calls after a warm-up; the chunks rotate through 64 different arrays and the buffer is emptied whenever 30 s are full, as tools/capture_probe.py
does. --kernel-stats merges the kernels' own durations from the stats of a kernel-trace run of --kernels-only; --kernel-trace splits that run's dispatches by
configuration and chunk length (the run's order is this file's: per configuration 250 warm-up appends of each kernel, then per chunk length 50 warm-up calls and
--trace-calls timed ones) and gives the median of each group; with --merge-into the figures go into an existing result and nothing is measured. Prints one JSON line."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AUDIO_MS = (10, 100, 1000)
CAP = 30 * 16000 + 16000 + 1024
ROTATE = 64
S16, F32 = 1, 4
CONFIGS = [dict(name="48000 Hz s16 mono", rate=48000, fmt=S16, channels=1, keep=0), dict(name="44100 Hz f32 stereo kept", rate=44100, fmt=F32, channels=2, keep=1)]


def speech_like(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-0.5, 0.5, n) * (0.002 + (np.sin(2 * np.pi * np.arange(n) / (16000 * 0.9)) > -0.3))).astype(np.float32)


def chunks_of(frames, fmt, channels):
    out = []
    for i in range(ROTATE):
        x = np.stack([speech_like(frames, 10 + 2 * i + c) for c in range(channels)], axis=1)
        out.append(np.ascontiguousarray(np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16) if fmt == S16 else x))
    return out


def appends(binding, h, src, fmt, calls, warmup=50):
    L = binding.lib()
    frames = len(src[0])
    feat = np.empty((frames * 16 // 256 + 4, 3), np.float32)
    n_new, size = C.c_int64(), C.c_int64()
    wall = []
    binding.check(L.wh_capture_clear(h))
    for i in range(warmup + calls):
        binding.check(L.wh_capture_size(h, C.byref(size)))
        if size.value > 30 * 16000 - 16001:
            binding.check(L.wh_capture_clear(h))
        a = src[i % ROTATE]
        t0 = time.perf_counter()
        rc = L.wh_capture_append(h, a.ctypes.data_as(C.c_void_p), fmt, frames, feat.ctypes.data_as(C.c_void_p), len(feat), C.byref(n_new))
        t1 = time.perf_counter()
        binding.check(rc)
        if i >= warmup:
            wall.append(t1 - t0)
    return wall


def stats(wall):
    us = np.asarray(wall) * 1e6
    return dict(median_us=float(np.median(us)), p10_us=float(np.percentile(us, 10)), p90_us=float(np.percentile(us, 90)), calls=len(us))


def kernel_stats(path):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for name in ("captureRateKernel", "captureAppendKernel"):
                if name in row.get("Name", ""):
                    out.setdefault(name, []).append(dict(name=row["Name"][:80], calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3,
                                                         min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3))
    out["source"] = "rocprofv3 --kernel-trace --stats over --kernels-only: both configurations and all three chunk lengths together"
    return out


def kernel_trace(path, calls):
    """medians of the traced dispatches per (configuration, chunk length): {kernel: {configuration: {audio_ms: median_us}}}"""
    with open(path, newline="") as f:
        rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    out = {}
    for name in ("captureRateKernel", "captureAppendKernel"):
        d = [ns for _, ns, k in rows if name in k]
        if len(d) != len(CONFIGS) * (250 + len(AUDIO_MS) * (50 + calls)):
            raise SystemExit("capture_rate_probe: %d dispatches of %s do not match --trace-calls %d" % (len(d), name, calls))
        i, out[name] = 0, {}
        for cfg in CONFIGS:
            i += 250
            out[name][cfg["name"]] = {}
            for ms in AUDIO_MS:
                out[name][cfg["name"]][str(ms)] = float(np.median(d[i + 50:i + 50 + calls])) / 1e3
                i += 50 + calls
    out["source"] = "rocprofv3 --kernel-trace over --kernels-only --calls %d: median duration of the timed dispatches of each group, us" % calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--kernel-trace", default="")
    ap.add_argument("--trace-calls", type=int, default=100)
    ap.add_argument("--merge-into", default="")
    a = ap.parse_args()
    if a.merge_into:
        with open(a.merge_into) as f:
            res = json.load(f)
        res["kernel_by_chunk"] = kernel_trace(a.kernel_trace, a.trace_calls)
        with open(a.merge_into, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res["kernel_by_chunk"]))
        return
    from whisper_amd import binding, ggml_format as gf
    if binding.device_count() < 1:
        raise SystemExit("capture_rate_probe: no GPU")
    L = binding.lib()
    m = binding.HipModel.from_ggml(gf.synth_model("test-d128", seed=1))
    ctx = binding.HipContext(m, 1)
    res = dict(rotate=ROTATE, configurations={})
    for cfg in CONFIGS:
        at_rate, at_16k = C.c_void_p(), C.c_void_p()
        binding.check(L.wh_capture_create_rate(ctx.handle, cfg["channels"], cfg["keep"], CAP, cfg["rate"], C.byref(at_rate)))
        binding.check(L.wh_capture_create(ctx.handle, cfg["channels"], cfg["keep"], CAP, C.byref(at_16k)))
        # warm the clocks and the first-use tables (the taps of the rate, the twiddles)
        appends(binding, at_rate, chunks_of(cfg["rate"] // 10, cfg["fmt"], cfg["channels"]), cfg["fmt"], 200)
        appends(binding, at_16k, chunks_of(1600, cfg["fmt"], cfg["channels"]), cfg["fmt"], 200)
        rows = {}
        for ms in AUDIO_MS:
            r = stats(appends(binding, at_rate, chunks_of(cfg["rate"] * ms // 1000, cfg["fmt"], cfg["channels"]), cfg["fmt"], a.calls))
            b = stats(appends(binding, at_16k, chunks_of(16 * ms, cfg["fmt"], cfg["channels"]), cfg["fmt"], a.calls))
            rows[str(ms)] = dict(audio_ms=ms, frames=cfg["rate"] * ms // 1000, at_rate=r, at_16k=b, rate_over_16k=r["median_us"] / b["median_us"])
        res["configurations"][cfg["name"]] = rows
        binding.check(L.wh_capture_destroy(at_rate))
        binding.check(L.wh_capture_destroy(at_16k))
    ctx.close()
    m.close()
    if a.kernels_only:
        return
    if a.kernel_stats:
        res["kernel"] = kernel_stats(a.kernel_stats)
    if a.kernel_trace:
        res["kernel_by_chunk"] = kernel_trace(a.kernel_trace, a.trace_calls)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
