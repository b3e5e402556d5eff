"""The dequantization kernel on the device, and what a quantized model file costs to load.

    python tools/dequant_probe.py [--out profiles/dequant_probe.json] [--launches 30] [--no-load]

wh_dequantize (whisper_amd/csrc/dequant.hip) on the token embedding of the released multilingual models up to medium, 51865 x 1024, for each of the five
block types: hip-event time per launch, warm-up first, median of --launches launches; the inputs rotate through buffers that together exceed the last-level
cache (512 MB), so that no launch finds its blocks there. Next to it the yardstick the kernel is held against: the host-to-device copy of the same payload
(pageable and pinned host memory), which the loader pays anyway.
Then the wall time of loadModel (api.Model: libWhisper.so, loadGgmlFile) on a medium-shape model with random weights, written as q5_0 and as its F16 twin
(the file whose arena is the same bytes): median of three loads each, the files in the page cache. No threshold is set: the yardstick of the load is the F16
file's time. Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROTATE_BYTES = 512 << 20
ROWS, COLS = 51865, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--no-load", action="store_true", help="the kernel only")
    a = ap.parse_args()
    import torch
    from whisper_amd import api, binding, ggml_format as gf
    L = binding.lib()
    if not torch.cuda.is_available():
        raise SystemExit("dequant_probe: no GPU")
    n_blocks = ROWS * COLS // 32
    res = dict(launches=a.launches, rotate_mb=ROTATE_BYTES >> 20, rows=ROWS, cols=COLS, blocks=n_blocks, output_mb=n_blocks * 64 / 1e6, kernel={})
    rng = np.random.default_rng(1)
    dst = torch.empty(n_blocks * 32, dtype=torch.float16, device="cuda")
    for qtype, type_id in gf.GGML_TYPES.items():
        size = gf.BLOCK_BYTES[qtype]
        host = rng.integers(0, 256, n_blocks * size, dtype=np.uint8)
        host.reshape(n_blocks, size)[:, 1] &= 0x3F                               # finite scales of ordinary size
        n_buf = ROTATE_BYTES // host.nbytes + 2
        first = torch.from_numpy(host).cuda()
        bufs = [first] + [first.clone() for _ in range(n_buf - 1)]

        def launch(x):
            binding.check(L.wh_dequantize(None, type_id, C.c_void_p(x.data_ptr()), n_blocks, C.c_void_p(dst.data_ptr())))

        def timed(fn, count, warmup):
            for i in range(warmup):
                fn(i)
            torch.cuda.synchronize()
            us = []
            for i in range(count):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(warmup + i)
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            return us

        us = timed(lambda i: launch(bufs[i % n_buf]), a.launches, 5)
        r = dict(block_bytes=size, payload_mb=host.nbytes / 1e6, buffers=n_buf, kernel_us=float(np.median(us)), kernel_us_min=float(np.min(us)), kernel_us_max=float(np.max(us)))
        r["read_plus_write_gb_s"] = (host.nbytes + n_blocks * 64) / r["kernel_us"] * 1e-3
        # the yardstick: the same payload host -> device
        pageable, pinned = torch.from_numpy(host), torch.from_numpy(host).pin_memory()
        for name, src in (("h2d_pageable_us", pageable), ("h2d_pinned_us", pinned)):
            r[name] = float(np.median(timed(lambda i: bufs[i % n_buf].copy_(src, non_blocking=True), 7, 2)))
        # the result is the restatement's (the first rows: the whole check is the test suite's)
        launch(first)
        torch.cuda.synchronize()
        want = gf.dequantize_f16(gf.QTensor(qtype, (4096, 32), host[:4096 * size]))
        assert np.array_equal(dst[:4096 * 32].cpu().numpy().view(np.uint16), want.view(np.uint16).reshape(-1))
        res["kernel"][qtype] = r
        del bufs, first, pinned
        torch.cuda.empty_cache()
    del dst
    torch.cuda.empty_cache()

    if not a.no_load:
        t0 = time.perf_counter()
        model = gf.synth_model("medium", seed=3)
        qm = gf.quantize_model(model, "q5_0")
        twin = gf.dequantized_twin(qm)
        del model
        load = dict(model="medium shape, random weights", prepare_s=0.0, files={})
        with tempfile.TemporaryDirectory() as tmp:
            for name, m in (("q5_0", qm), ("f16_twin", twin)):
                path = os.path.join(tmp, name + ".bin")
                size = gf.write_model(path, m)
                load["files"][name] = dict(file_mb=size / 1e6)
            del qm, twin
            load["prepare_s"] = time.perf_counter() - t0
            for name in ("f16_twin", "q5_0", "f16_twin", "q5_0", "f16_twin", "q5_0", "f16_twin", "q5_0"):        # alternating; the first pair is warm-up
                path = os.path.join(tmp, name + ".bin")
                t0 = time.perf_counter()
                m = api.Model(path)
                dt = time.perf_counter() - t0
                m.close()
                load["files"][name].setdefault("load_s_all", []).append(dt)
        for f in load["files"].values():
            f["load_s"] = float(np.median(f["load_s_all"][1:]))
        load["q5_0_over_f16"] = load["files"]["q5_0"]["load_s"] / load["files"]["f16_twin"]["load_s"]
        res["load"] = load
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
