"""INT8 encoder products against the FP16 ones, product by product (DESIGN.md section 7 "INT8 encoder products"), at the medium shape: d = 1024, 16 heads,
M = 64 windows x 1500 rows.

  qkv / out / up / down   the product as wh_encode builds it, through wh_op_gemm_encoder (the FP16 kernel the chooser picks) and wh_op_gemm_encoder_i8 (gemmI8),
                          alternating in ONE process, hip events around every launch, the median of 30; the operands rotate over three sets (A alone is 98 .. 786 MB
                          per set), so no launch finds its rows in the Infinity Cache. With it the quantizer pass the INT8 product needs in front of it: layerNormI8
                          against layerNorm (qkv, up), quantizeRowsI8 (out, down; TB/s over 2 K bytes read and K + 4 written per row).
  encode                  one wh_encode of 64 windows on a context with the setting and on one without (an arena of constant FP16 weights: the time does not depend
                          on the values), alternating, the host's clock around encode + synchronize, the median of 10.

The ratio printed next to each product is INT8 time (product + what its quantizer pass adds) over FP16 time; `predicted` is the a nk + b model of DESIGN.md
section 8.3 with half the K tiles. Every step is a child process under its own time limit; a failing step ends the probe.

    python tools/encoder_i8_probe.py            # prints one JSON line and writes it to profiles/encoder_i8_probe.json
"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, H, T, WINDOWS, REPS, SETS = 1024, 16, 1500, 64, 30, 3
M = WINDOWS * T
# name -> ( N, K, epi, predicted time ratio )
PRODUCTS = {"qkv": (3 * D, D, 3, 0.60), "out": (D, D, 0, 0.70), "up": (4 * D, D, 1, 0.60), "down": (D, 4 * D, 0, 0.57)}


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
    N, K, epi, predicted = PRODUCTS[name]
    a16 = [(0.5 * torch.randn((M, K), device="cuda")).half() for _ in range(SETS)]
    w16 = (torch.randn((N, K), device="cuda") / K ** 0.5).half()
    bias = 0.1 * torch.randn(N, device="cuda")
    a8, sa = torch.empty((SETS, M, K), dtype=torch.int8, device="cuda"), torch.empty((SETS, M), device="cuda")
    w8, sw = torch.empty((N, K), dtype=torch.int8, device="cuda"), torch.empty(N, device="cuda")
    for i in range(SETS):
        B.check(L.wh_op_quantize_rows_i8(None, p(a16[i]), K, p(a8[i]), p(sa[i]), M, K))
    B.check(L.wh_op_quantize_rows_i8(None, p(w16), K, p(w8), p(sw), N, K))
    f = dict(M=M, N=N, K=K, lda=K, Mb=M, ldc=N, epi=epi, bias=bias.data_ptr())
    if epi == 0:
        x = torch.randn((M, N), device="cuda")
        f.update(out32=x.data_ptr(), res=x.data_ptr())
    elif epi == 1:
        h = torch.empty((M, N), dtype=torch.float16, device="cuda")
        f.update(out16=h.data_ptr())
    else:
        q, k, v = (torch.zeros((WINDOWS, H, T + 36, 64), dtype=torch.float16, device="cuda") for _ in range(3))
        f.update(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), T=T, Tpad=T + 36, H=H, B=WINDOWS)
    calls = {"fp16": lambda i: B.op_gemm_encoder(a=a16[i % SETS].data_ptr(), w=w16.data_ptr(), scale=1.0, **f),
             "int8": lambda i: B.op_gemm_encoder_i8(p(sa[i % SETS]), p(sw), a=a8[i % SETS].data_ptr(), w=w8.data_ptr(), **f)}
    if name in ("qkv", "up"):                                                  # the LayerNorm in front: what writing int8 + scales costs over writing FP16
        xs = [torch.randn((M, D), device="cuda") for _ in range(SETS)]
        lw, lb, o16 = 1 + 0.1 * torch.randn(D, device="cuda"), 0.1 * torch.randn(D, device="cuda"), torch.empty((M, D), dtype=torch.float16, device="cuda")
        calls["ln16"] = lambda i: B.check(L.wh_op_layer_norm(None, p(xs[i % SETS]), p(lw), p(lb), p(o16), M, D))
        calls["ln8"] = lambda i: B.check(L.wh_op_layer_norm_i8(None, p(xs[i % SETS]), p(lw), p(lb), p(a8[0]), p(sa[0]), M, D))
    else:
        calls["quant"] = lambda i: B.check(L.wh_op_quantize_rows_i8(None, p(a16[i % SETS]), K, p(a8[0]), p(sa[0]), M, K))
    us = _median_us(calls)
    extra = us["ln8"] - us["ln16"] if "ln8" in us else us["quant"]
    rec = {name + "_" + k + "_us": round(v, 1) for k, v in us.items()}
    if "quant" in us:
        rec[name + "_quant_tbs"] = round(M * (3.0 * K + 4) / us["quant"] / 1e6, 3)
    rec.update({name + "_fp16_tflops": round(2.0 * M * N * K / us["fp16"] / 1e6, 1), name + "_int8_tops": round(2.0 * M * N * K / us["int8"] / 1e6, 1),
                name + "_kernel_ratio": round(us["int8"] / us["fp16"], 3), name + "_ratio_with_quantizer": round((us["int8"] + extra) / us["fp16"], 3),
                name + "_predicted": predicted})
    return rec


def encode():
    import torch
    from whisper_amd import binding as B, ggml_format as gf
    hp = gf.hparams_for("medium")
    arena = torch.full((B.arena_bytes(hp) // 2,), 0x2C00, dtype=torch.int16, device="cuda")       # FP16 0.0625 everywhere; finite as FP32 pairs too
    m = B.HipModel(hp, arena_ptr=arena.data_ptr(), already_filled=True, keepalive=arena)
    mel = torch.rand((WINDOWS, hp.n_mels, 3000), device="cuda") * 2 - 1
    c16, c8 = B.HipContext(m, WINDOWS), B.HipContext(m, WINDOWS)
    c8.set_encoder_i8(True)
    # a context runs on its own stream: the host's clock around encode + synchronize (100 ms and more per call, so the launch overhead does not matter)
    ms = {"fp16": [], "int8": []}
    for i in range(12):
        for n, c in (("fp16", c16), ("int8", c8)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.encode(mel)
            c.synchronize()
            if i >= 2:
                ms[n].append((time.perf_counter() - t0) * 1e3)
    med = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}
    return {"encode64_fp16_ms": round(med["fp16"], 2), "encode64_int8_ms": round(med["int8"], 2), "encode64_ratio": round(med["int8"] / med["fp16"], 3)}


def main():
    if len(sys.argv) == 2:
        print(json.dumps(encode() if sys.argv[1] == "encode" else product(sys.argv[1])))
        return 0
    rec = {"probe": "encoder_i8", "d": D, "rows": M, "reps": REPS}
    for step in list(PRODUCTS) + ["encode"]:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), step], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print("step %s ended with status %d: nothing more is started" % (step, r.returncode), file=sys.stderr)
            return 1
        rec.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(rec)
    print(line)
    with open(os.path.join(ROOT, "profiles", "encoder_i8_probe.json"), "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
