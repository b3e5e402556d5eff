"""What the speech-only filter costs, and what it saves.

    python tools/speech_only_probe.py [--out profiles/speech_only_probe.json] [--launches 20] [--kernel-stats kernel_stats.csv] [--cli MODEL.bin]
    python tools/speech_only_probe.py --kernels-only          # the launches alone, for a kernel-trace run of their own (rocprofv3 --kernel-trace --stats)

1. The pack kernel (whisper_amd/csrc/speech.hip) at one hour of 16 kHz mono float32 with half of it kept in spans of 2 s (every other 2 s: 900 spans of 125
   frames, 115.2 MB read and 115.2 MB written): hip-event time around one wh_speech_pack call -- which also allocates, uploads and frees its span table and
   waits for the stream -- and around a device-to-device hipMemcpy of the same byte count in the same run; medians of --launches after a warm-up, the sources
   rotating through buffers that together exceed the last-level cache.
2. --kernel-stats: the kernel's own duration, read from the stats of a kernel-trace run of --kernels-only (a run of its own, no counters), merged in with
   its ratio to the copy.
3. --cli MODEL.bin: the wall time of whisper-main on the tests' composite recording (39.1 s of which 30.06 s are speech) repeated to several minutes, with and
   without --speech-only, three runs each; the model is whatever file is named (the figures say which).
Prints one JSON line."""
import argparse
import csv
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SECONDS, SPAN_S = 3600, 2
ROTATE_BYTES = 512 << 20


def pack_case():
    n = 16000 * SECONDS
    spans = np.asarray([(16000 * s, 16000 * (s + SPAN_S)) for s in range(0, SECONDS, 2 * SPAN_S)], np.int64)
    assert (spans % 256 == 0).all()
    return n, spans, int((spans[:, 1] - spans[:, 0]).sum())


def pack_launches(launches, timed):
    import torch
    from whisper_amd import binding
    L = binding.lib()
    n, spans, n_out = pack_case()
    host = np.random.default_rng(1).uniform(-0.5, 0.5, n).astype(np.float32)
    n_buf = ROTATE_BYTES // host.nbytes + 2
    first = torch.from_numpy(host).cuda()
    bufs = [first] + [first.clone() for _ in range(n_buf - 1)]
    dst = torch.empty(n_out, dtype=torch.float32, device="cuda")

    def kernel(x):
        binding.check(L.wh_speech_pack(None, C.c_void_p(x.data_ptr()), 1, n, spans.ctypes.data_as(C.c_void_p), len(spans), C.c_void_p(dst.data_ptr()), n_out))

    def copy(x):
        dst.copy_(x[:n_out])

    out = {}
    for name, fn in (("pack", kernel), ("memcpy_dtod", copy)):
        for i in range(5):
            fn(bufs[i % n_buf])
        torch.cuda.synchronize()
        us = []
        for i in range(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(bufs[(5 + i) % n_buf])
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        out[name] = dict(median_us=float(np.median(us)), min_us=float(np.min(us)), max_us=float(np.max(us)), calls=launches)
    if timed:
        kernel(first)
        torch.cuda.synchronize()
        want = np.concatenate([host[a:b] for a, b in spans])
        assert np.array_equal(dst.cpu().numpy().view(np.uint32), want.view(np.uint32))
    bytes_moved = 2 * 4 * n_out
    for r in out.values():
        r["gb_s"] = bytes_moved / r["median_us"] * 1e-3
    out["pack_over_memcpy_event_time"] = out["pack"]["median_us"] / out["memcpy_dtod"]["median_us"]
    return dict(seconds=SECONDS, span_seconds=SPAN_S, spans=len(spans), samples_kept=n_out, bytes_read_and_written=bytes_moved, buffers=n_buf, **out)


def kernel_stats(path, res):
    """the row of the pack kernel in rocprofv3's kernel stats (names and columns as the tool writes them: Name, Calls, TotalDurationNs, AverageNs, MinNs, MaxNs)"""
    with open(path) as f:
        for row in csv.DictReader(f):
            if "speechPackKernel" in row.get("Name", ""):
                res["kernel"] = dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) * 1e-3, min_us=float(row["MinNs"]) * 1e-3, max_us=float(row["MaxNs"]) * 1e-3,
                                     source="rocprofv3 --kernel-trace --stats over --kernels-only")
                res["kernel"]["gb_s"] = res["pack"]["bytes_read_and_written"] / res["kernel"]["average_us"] * 1e-3
                res["kernel"]["over_memcpy_dtod_event_time"] = res["kernel"]["average_us"] / res["pack"]["memcpy_dtod"]["median_us"]
                return
    raise SystemExit("speech_only_probe: no speechPackKernel row in " + path)


def cli_times(model, repeats=8, runs=3):
    import importlib.util
    import vad_ref as V
    from whisper_amd import build
    spec = importlib.util.spec_from_file_location("make_golden_runfull", os.path.join(ROOT, "tests", "golden", "make_golden_runfull.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    pieces = [mg.pcm_for("jfk"), mg.pcm_for("mixed")[:int(9.3 * 16000)], mg.pcm_for("jfk")[:6 * 16000]]
    raw, _ = V.composite(pieces, [3.0, 4.5, 2.6], 40, lead=2.7)
    q = np.tile(np.clip(np.round(raw * 32768.0), -32768, 32767).astype("<i2"), repeats)
    out = dict(model=os.path.basename(model), audio_seconds=len(q) / 16000.0, runs=runs)
    with tempfile.TemporaryDirectory() as tmp:
        wav = os.path.join(tmp, "rec.wav")
        with wave.open(wav, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(q.tobytes())
        for name, extra in (("plain", []), ("speech_only", ["--speech-only"])):
            wall, segments = [], 0
            for _ in range(runs):
                t0 = time.perf_counter()
                r = subprocess.run([build.CLI_BIN, "-m", model, "-f", wav, "-l", "en", "-nc"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
                wall.append(time.perf_counter() - t0)
                if r.returncode != 0:
                    raise SystemExit("speech_only_probe: whisper-main failed: " + r.stderr.decode(errors="replace")[-500:])
                segments = sum(1 for ln in r.stdout.splitlines() if b" --> " in ln)
            out[name] = dict(wall_s=[float(x) for x in wall], median_s=float(np.median(wall)), segments=segments)
    out["speech_only_over_plain"] = out["speech_only"]["median_s"] / out["plain"]["median_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--cli", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("speech_only_probe: no GPU")
    if a.kernels_only:
        pack_launches(a.launches, False)
        return
    res = dict(pack=pack_launches(a.launches, True))
    if a.kernel_stats:
        kernel_stats(a.kernel_stats, res)
    if a.cli:
        res["whisper_main"] = cli_times(a.cli)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
