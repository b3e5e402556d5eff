"""INT8 decoder weights against the FP16 decode-step products (DESIGN.md section 7 "INT8 decoder weights"), at the medium decoder's shapes.

  products   one gemvW8 launch (wh_op_gemv_w8) against the launch the FP16 path takes for the same shape (wh_op_mul_mat / wh_op_mul_mat_gelu: launchGemv's choice),
             alternating in ONE process, hip events around every launch, the median of 40. Shapes N x K: 3072 x 1024 (Q/K/V; FP32 epilogue here), 1024 x 1024
             (attention out), 4096 x 1024 (MLP up, GELU epilogue), 1024 x 4096 (MLP down), 51865 x 1024 (vocabulary), each at 1, 8, 32, 64 and 128 rows. The weights
             rotate over enough copies (768 MB of FP16, the same number of int8 copies) that no launch finds its rows in the Infinity Cache, as in a decode step,
             whose layers stream 600 MB between two uses of a matrix.
  step       64 steps of the device-side greedy loop (wh_decode_greedy: captured graphs, sampler included) at 8 and 32 sequences on a context with the setting
             and on one without (an arena of constant FP16 weights: the time does not depend on the values), alternating, the host's clock around the call, the
             median of 7, per step.

Every step is a child process under its own time limit; a failing step ends the probe.

    python tools/decoder_w8_probe.py            # prints one JSON line and writes it to profiles/decoder_w8_probe.json
"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, ROWS, FP16_BYTES = 40, (1, 8, 32, 64, 128), 768 << 20
# name -> ( N, K, GELU epilogue )
SHAPES = {"qkv": (3072, 1024, False), "out": (1024, 1024, False), "up": (4096, 1024, True), "down": (1024, 4096, False), "vocab": (51865, 1024, False)}


def _median_us(calls, reps=REPS):
    import torch
    for i in range(3):
        for fn in calls.values():
            fn(i)
    torch.cuda.synchronize()
    ev = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for n in calls}
    for i in range(reps):
        for n, fn in calls.items():
            ev[n][i][0].record()
            fn(i)
            ev[n][i][1].record()
    torch.cuda.synchronize()
    return {n: sorted(a.elapsed_time(b) * 1e3 for a, b in ev[n])[reps // 2] for n in calls}


def product(name):
    import torch
    from whisper_amd import binding as B
    L = B.lib()
    p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    N, K, gelu = SHAPES[name]
    sets = max(3, FP16_BYTES // (2 * N * K))
    w16 = (torch.randn((sets, N, K), device="cuda") / K ** 0.5).half()
    w8, sw = torch.empty((sets, N, K), dtype=torch.int8, device="cuda"), torch.empty((sets, N), device="cuda")
    for s in range(sets):
        B.check(L.wh_op_quantize_rows_i8(None, p(w16[s]), K, p(w8[s]), p(sw[s]), N, K))
    bias = 0.1 * torch.randn(N, device="cuda")
    rec = {}
    for M in ROWS:
        a = torch.randn((M, K), device="cuda").half()
        x = torch.randn((M, N), device="cuda")
        h = torch.empty((M, N), dtype=torch.float16, device="cuda")
        if gelu:
            calls = {"fp16": lambda i: B.check(L.wh_op_mul_mat_gelu(None, p(a), p(w16[i % sets]), p(bias), p(h), M, N, K)),
                     "int8": lambda i: B.op_gemv_w8(M, N, K, p(w8[i % sets]), p(sw[i % sets]), epi=1, a=p(a), bias=p(bias), out16=p(h))}
        else:
            calls = {"fp16": lambda i: B.check(L.wh_op_mul_mat(None, p(a), p(w16[i % sets]), p(bias), p(x), p(x), M, N, K)),
                     "int8": lambda i: B.op_gemv_w8(M, N, K, p(w8[i % sets]), p(sw[i % sets]), a=p(a), bias=p(bias), res=p(x), out32=p(x))}
        us = _median_us(calls)
        rec["%s_m%d" % (name, M)] = {"fp16_us": round(us["fp16"], 2), "int8_us": round(us["int8"], 2), "ratio": round(us["int8"] / us["fp16"], 3),
                                     "fp16_gbs": round(2.0 * N * K / us["fp16"] / 1e3, 1), "int8_gbs": round(1.0 * N * K / us["int8"] / 1e3, 1)}
    return rec


def step(seqs):
    import numpy as np
    import torch
    from whisper_amd import binding as B, ggml_format as gf
    hp = gf.hparams_for("medium")
    arena = torch.full((B.arena_bytes(hp) // 2,), 0x2C00, dtype=torch.int16, device="cuda")       # FP16 0.0625 everywhere; finite as FP32 pairs too
    m = B.HipModel(hp, arena_ptr=arena.data_ptr(), already_filled=True, keepalive=arena)
    mel = torch.rand((seqs, hp.n_mels, 3000), device="cuda") * 2 - 1
    c16, c8 = B.HipContext(m, seqs), B.HipContext(m, seqs)
    c8.set_decoder_w8(True)
    steps, ms = 64, {"fp16": [], "int8": []}
    first = np.full(seqs, gf.special_tokens(hp)["sot"], np.int32)
    for c in (c16, c8):
        c.encode(mel)
    for i in range(9):
        for n, c in (("fp16", c16), ("int8", c8)):
            c.synchronize()
            t0 = time.perf_counter()
            c.decode_greedy(first, 0, steps)
            if i >= 2:
                ms[n].append((time.perf_counter() - t0) * 1e3 / steps)
    med = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}
    return {"step%d_fp16_us" % seqs: round(med["fp16"] * 1e3, 1), "step%d_int8_us" % seqs: round(med["int8"] * 1e3, 1), "step%d_ratio" % seqs: round(med["int8"] / med["fp16"], 3)}


def main():
    if len(sys.argv) == 2:
        print(json.dumps(step(int(sys.argv[1][4:])) if sys.argv[1].startswith("step") else product(sys.argv[1])))
        return 0
    rec = {"probe": "decoder_w8", "reps": REPS}
    for name in list(SHAPES) + ["step8", "step32"]:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), name], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print("step %s ended with status %d: nothing more is started" % (name, r.returncode), file=sys.stderr)
            return 1
        rec.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(rec)
    print(line)
    with open(os.path.join(ROOT, "profiles", "decoder_w8_probe.json"), "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
