"""The resampling kernel on the device, and what the same work costs on one host thread.

    python tools/resample_probe.py [--out profiles/resample_probe.json] [--launches 30] [--no-host]

wh_resample (whisper_amd/csrc/resample.hip) on 30 s and 200 s of 44.1 kHz stereo s16 (mean of the channels), 48 kHz mono float32 and 11.025 kHz mono s16
(640 phases: the table staged in chunks of 11 taps), each with the taps staged through LDS and read from global memory: hip-event
time per launch, warm-up first, median of --launches launches; the inputs rotate through buffers that together exceed the last-level cache (512 MB),
so that no launch finds its samples there. Next to it the wall time of wh_resample_host (upload of the file's own samples, kernel, download; pageable
host memory) and of scipy.signal.resample_poly on one host thread for the same conversion (its default Kaiser window: a shorter filter than the
kernel's, so the host figure is a lower bound). The yardstick: at the headline rate a 200 s clip is 18.9 ms of GPU time; the kernel should stay
under 1 % of that, 190 us. Prints one JSON line."""
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
S16, F32 = 1, 4             # wh_pcm_format
CASES = [("44100_stereo_s16", 44100, 2, S16), ("48000_mono_f32", 48000, 1, F32), ("11025_mono_s16", 11025, 1, S16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--no-host", action="store_true", help="skip scipy.signal.resample_poly")
    a = ap.parse_args()
    import torch
    from whisper_amd import binding
    L = binding.lib()
    if not torch.cuda.is_available():
        raise SystemExit("resample_probe: no GPU")
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    res = dict(launches=a.launches, rotate_mb=ROTATE_BYTES >> 20, yardstick_us_200s=190.0, cases={})
    rng = np.random.default_rng(1)
    for name, rate, channels, fmt in CASES:
        for seconds in (30, 200):
            frames = rate * seconds
            n_out = C.c_int64()
            binding.check(L.wh_resample_out_len(rate, frames, C.byref(n_out)))
            n_out = n_out.value
            if fmt == S16:
                host = rng.integers(-20000, 20000, (frames, channels)).astype(np.int16)
            else:
                host = rng.uniform(-0.6, 0.6, (frames, channels)).astype(np.float32)
            n_buf = ROTATE_BYTES // host.nbytes + 2
            first = torch.from_numpy(host).cuda()
            bufs = [first] + [first.clone() for _ in range(n_buf - 1)]
            dst = torch.empty(n_out, dtype=torch.float32, device="cuda")

            def launch(x):
                binding.check(L.wh_resample(None, C.c_void_p(x.data_ptr()), fmt, channels, -1, rate, frames, C.c_void_p(dst.data_ptr()), 1, n_out))

            warmup = 5

            def timed():
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
                return us

            us = timed()
            # A/B: the same launches with the taps read from global memory instead of staged through LDS (option "resample_lds_phases" = 0)
            binding.set_option("resample_lds_phases", 0)
            try:
                us_global = timed()
            finally:
                binding.set_option("resample_lds_phases", binding.get_option_default("resample_lds_phases"))
            taps = [C.c_int32() for _ in range(4)]
            binding.check(L.wh_resample_taps(rate, *[C.byref(t) for t in taps], None, 0))
            K = taps[3].value
            r = dict(seconds=seconds, frames=frames, n_out=n_out, taps_per_output=K, buffers=n_buf, kernel_us=float(np.median(us)), kernel_us_min=float(np.min(us)),
                     kernel_us_max=float(np.max(us)))
            r["kernel_us_taps_from_global"] = float(np.median(us_global))
            r["gflop_s"] = 2.0 * K * n_out / r["kernel_us"] * 1e-3
            r["input_gb_s"] = host.nbytes / r["kernel_us"] * 1e-3
            # host -> host: upload, kernel, download
            out = np.empty(n_out, np.float32)
            wall = []
            for i in range(4):
                t0 = time.perf_counter()
                binding.check(L.wh_resample_host(host.ctypes.data_as(C.c_void_p), fmt, channels, -1, rate, frames, out.ctypes.data_as(C.c_void_p), 1, n_out))
                wall.append(time.perf_counter() - t0)
            r["host_entry_ms"] = float(np.median(wall[1:])) * 1e3
            torch.cuda.synchronize()
            assert np.array_equal(out, dst.cpu().numpy())      # every rotated buffer holds the same samples
            if not a.no_host:
                from scipy import signal
                x = host.astype(np.float32)
                x = x.mean(1) if fmt == F32 else x.mean(1) / np.float32(32768.0)
                g = np.gcd(rate, 16000)
                t0 = time.perf_counter()
                y = signal.resample_poly(x, 16000 // g, rate // g)
                r["scipy_resample_poly_ms_one_thread"] = (time.perf_counter() - t0) * 1e3
                r["scipy_max_abs_difference"] = float(np.abs(y[2000:n_out - 2000] - out[2000:len(y) - 2000]).max()) if len(y) == n_out else None
            res["cases"]["%s_%ds" % (name, seconds)] = r
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
