"""The voice-activity feature kernel on the device, and what the rest of a split costs.

    python tools/vad_probe.py [--out profiles/vad_probe.json] [--launches 30]

wh_vad_features (whisper_amd/csrc/vad.hip) on 200 s and 3600 s of 16 kHz mono float32: hip-event time per launch, warm-up first, median of --launches
launches; the inputs rotate through buffers that together exceed the last-level cache (512 MB), so that no launch finds its samples there. Next to it
the wall time of wh_vad_features_host (upload, kernel, download; pageable host memory), of the decision loop plus the planner on the host
(api.plan_chunks minus the features) and of the whole api.plan_chunks call. The yardstick: at the headline rate a 200 s clip is 18.9 ms of GPU time;
the kernel should stay under 1 % of that, 190 us. Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROTATE_BYTES = 512 << 20
CLIP_200S_MS = 18.9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=30)
    a = ap.parse_args()
    import torch
    from whisper_amd import api, binding
    L = binding.lib()
    if not torch.cuda.is_available():
        raise SystemExit("vad_probe: no GPU")
    res = dict(launches=a.launches, rotate_mb=ROTATE_BYTES >> 20, yardstick_us_200s=190.0, clip_200s_ms=CLIP_200S_MS, cases={})
    rng = np.random.default_rng(1)
    for seconds in (200, 3600):
        n = 16000 * seconds
        n_frames = n // 256
        # speech-like: bursts of noise between quiet spans, so that the planner finds pauses
        host = (rng.uniform(-0.5, 0.5, n) * (0.002 + (np.sin(2 * np.pi * np.arange(n) / (16000 * 3.7)) > -0.6))).astype(np.float32)
        n_buf = ROTATE_BYTES // host.nbytes + 2
        first = torch.from_numpy(host).cuda()
        bufs = [first] + [first.clone() for _ in range(n_buf - 1)]
        dst = torch.empty(3 * n_frames, dtype=torch.float32, device="cuda")

        def launch(x):
            binding.check(L.wh_vad_features(None, C.c_void_p(x.data_ptr()), n, C.c_void_p(dst.data_ptr())))

        warmup = 5
        for i in range(warmup):
            launch(bufs[i % n_buf])
        torch.cuda.synchronize()
        us = []
        for i in range(a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(bufs[(warmup + i) % n_buf])
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        r = dict(seconds=seconds, frames=n_frames, buffers=n_buf, kernel_us=float(np.median(us)), kernel_us_min=float(np.min(us)), kernel_us_max=float(np.max(us)))
        # bins 0 .. 127 as real and imaginary sums of 256 terms
        r["gflop_s"] = 2.0 * 2 * 128 * 256 * n_frames / r["kernel_us"] * 1e-3
        r["input_gb_s"] = host.nbytes / r["kernel_us"] * 1e-3
        r["share_of_transcription"] = r["kernel_us"] * 1e-3 / (CLIP_200S_MS * seconds / 200.0)
        feat = np.empty((n_frames, 3), np.float32)
        wall = []
        for i in range(4):
            t0 = time.perf_counter()
            binding.check(L.wh_vad_features_host(host.ctypes.data_as(C.c_void_p), n, feat.ctypes.data_as(C.c_void_p)))
            wall.append(time.perf_counter() - t0)
        r["host_entry_ms"] = float(np.median(wall[1:])) * 1e3
        torch.cuda.synchronize()
        assert np.array_equal(feat.reshape(-1), dst.cpu().numpy(), equal_nan=True)      # every rotated buffer holds the same samples
        t0 = time.perf_counter()
        speech, _ = api.vad_decide(feat)
        r["decide_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        plan = api.plan_chunks(host)
        r["plan_chunks_ms"] = (time.perf_counter() - t0) * 1e3
        r["chunks"] = len(plan)
        r["speech_share"] = float(speech.mean())
        res["cases"]["%ds" % seconds] = r
        del bufs, first, dst
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
