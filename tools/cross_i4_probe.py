"""INT4 cross-attention caches against the FP16 and the FP8 ones, kernel by kernel (DESIGN.md section 7 "INT4 cross-attention caches"):

  attention  attentionDecG<1, true> (FP16 caches), attentionDecG8<1, true> (E4M3 bytes + row scales) and attentionDecG4<1, true> (nibbles + row scales) on the
             headline decode step -- 448 and 112 windows x 16 heads x 1500 keys, d = 1024 -- alternating in ONE process, hip events around every launch, the
             median of 30; the inputs rotate over sets of caches whose bytes add up to more than the Infinity Cache for every format (the INT4 caches of 112
             windows are 0.19 GB a set: four sets), so no launch finds its rows there;
  quantize   quantizeCrossKV4 on one layer x 128 windows (K and V rows of one set).

Microseconds and achieved TB/s (algorithmic bytes: every K and V row once, scales included). The yardsticks are the FP16 and the FP8 kernel of the same run; the
byte ratios 36 / 128 and 36 / 68 per row are the floors of the time ratios. Every step is a child process under its own time limit; a failing step ends the probe.

    python tools/cross_i4_probe.py            # prints one JSON line and writes it to profiles/cross_i4_probe.json
"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("attention", 448), ("attention", 112), ("quantize", 128))
HEADS, KEYS, REPS = 16, 1500, 30


def _median_us(calls):
    """calls: {name: fn( i )}. Launches alternate between the names; returns {name: median us of REPS launches}."""
    import torch
    for i in range(3):
        for fn in calls.values():
            fn(i)
    torch.cuda.synchronize()
    ev = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)] for n in calls}
    for i in range(REPS):
        for n, fn in calls.items():
            ev[n][i][0].record()
            fn(i)
            ev[n][i][1].record()
    torch.cuda.synchronize()
    return {n: sorted(a.elapsed_time(b) * 1e3 for a, b in ev[n])[REPS // 2] for n in calls}


def step(kind, windows):
    import torch
    from whisper_amd import binding
    L = binding.lib()
    p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    d, blocks, rows, kb = HEADS * 64, windows * HEADS, windows * HEADS * KEYS, (KEYS + 63) // 64
    sets = 2 if windows >= 448 else 4

    def quant4(t):
        k, v = torch.empty((rows, 32), dtype=torch.uint8, device="cuda"), torch.empty((blocks * kb, 64, 32), dtype=torch.uint8, device="cuda")
        s = torch.empty(rows, dtype=torch.float32, device="cuda")
        return k, v, s

    if kind == "quantize":
        src = [(0.8 * torch.randn((rows, 64), device="cuda")).half() for _ in range(2)]
        k, v, s = quant4(src[0])
        us = _median_us({"quantize": lambda i: binding.check(L.wh_op_quantize_cross_kv_i4(None, p(src[i % 2]), p(k), None, p(s), blocks, KEYS)),
                         "quantize_kv": lambda i: binding.check(L.wh_op_quantize_cross_kv_i4(None, p(src[i % 2]), p(k), p(v), p(s), blocks, KEYS))})
        return {"quantize_rows": rows, "quantize_k_us": round(us["quantize"], 1), "quantize_k_tbs": round(rows * (128 + 32 + 4) / us["quantize"] / 1e6, 3),
                "quantize_kv_us": round(us["quantize_kv"], 1)}
    q8, q4, K, V = [], [], [], []
    for i in range(sets):
        k, v = (0.8 * torch.randn((windows, HEADS, KEYS, 64), device="cuda")).half(), torch.randn((windows, HEADS, KEYS, 64), device="cuda").half()
        set8, set4 = [], []
        for t, pick in ((k, 0), (v, 1)):
            b, s = torch.empty((rows, 64), dtype=torch.uint8, device="cuda"), torch.empty(rows, dtype=torch.float32, device="cuda")
            binding.check(L.wh_op_quantize_kv(None, p(t), p(b), p(s), rows))
            set8 += [b, s]
            n = quant4(t)
            binding.check(L.wh_op_quantize_cross_kv_i4(None, p(t), p(n[0]), p(n[1]), p(n[2]), blocks, KEYS))
            set4 += [n[pick], n[2]]
        q8.append(set8)
        q4.append(set4)
        if i < 2:                                   # the FP16 sets: two are 1.4 GB at 112 windows already
            K.append(k)
            V.append(v)
    x = torch.randn((windows, d), device="cuda") * 2 + 0.3
    lw, lb = 1 + 0.1 * torch.randn(d, device="cuda"), 0.1 * torch.randn(d, device="cuda")
    wq, bq = (torch.randn((d, d), device="cuda") / d ** 0.5).half(), 0.1 * torch.randn(d, device="cuda")
    out = torch.zeros((windows, d), device="cuda", dtype=torch.float16)
    scale = C.c_float(64.0 ** -0.25)
    us = _median_us({
        "fp16": lambda i: binding.check(L.wh_op_decoder_cross_attention(None, p(x), p(lw), p(lb), p(wq), p(bq), scale, p(K[i % 2]), p(V[i % 2]), p(out), windows, HEADS, KEYS, KEYS, 1)),
        "fp8": lambda i: binding.check(L.wh_op_decoder_cross_attention_f8(None, None, p(x), p(lw), p(lb), p(wq), p(bq), scale, *[p(t) for t in q8[i % sets]], p(out), windows, HEADS, 1, KEYS, KEYS, 1)),
        "i4": lambda i: binding.check(L.wh_op_decoder_cross_attention_i4(None, None, p(x), p(lw), p(lb), p(wq), p(bq), scale, *[p(t) for t in q4[i % sets]], p(out), windows, HEADS, 1, KEYS, KEYS, 1)),
    })
    n = "w%d" % windows
    return {n + "_fp16_us": round(us["fp16"], 1), n + "_fp16_tbs": round(2.0 * rows * 128 / us["fp16"] / 1e6, 3),
            n + "_fp8_us": round(us["fp8"], 1), n + "_fp8_tbs": round(2.0 * rows * 68 / us["fp8"] / 1e6, 3),
            n + "_i4_us": round(us["i4"], 1), n + "_i4_tbs": round(2.0 * rows * 36 / us["i4"] / 1e6, 3),
            n + "_i4_over_fp16": round(us["i4"] / us["fp16"], 3), n + "_i4_over_fp8": round(us["i4"] / us["fp8"], 3),
            "byte_ratio_fp16": round(36 / 128, 3), "byte_ratio_fp8": round(36 / 68, 3)}


def main():
    if len(sys.argv) == 3:
        print(json.dumps(step(sys.argv[1], int(sys.argv[2]))))
        return 0
    rec = {"probe": "cross_i4", "heads": HEADS, "keys": KEYS, "reps": REPS}
    for kind, windows in STEPS:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), kind, str(windows)], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print("step %s %d ended with status %d: nothing more is started" % (kind, windows, r.returncode), file=sys.stderr)
            return 1
        rec.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(rec)
    print(line)
    with open(os.path.join(ROOT, "profiles", "cross_i4_probe.json"), "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
