"""FP8 cross-attention caches against the FP16 ones, kernel by kernel (DESIGN.md section 7 "FP8 cross-attention caches"):

  attention  attentionDecG<1, true> (FP16 caches) and attentionDecG8<1, true> (E4M3 bytes + row scales) on the headline decode step -- 448 and 112 windows x 16
             heads x 1500 keys, d = 1024 -- alternating in ONE process, hip events around every launch, the median of 30; the inputs rotate over two sets of caches,
             each of which (0.69 .. 2.75 GB) is larger than the Infinity Cache, so no launch finds its rows there;
  quantize   quantizeCrossKV on one layer x 128 windows (K rows).

Microseconds and achieved TB/s (algorithmic bytes: every K and V row once, scales included). The yardstick is the FP16 kernel of the same run; the byte ratio
( 64 + 4 ) / 128 per row is the floor of the time ratio. Every step is a child process under its own time limit; a failing step ends the probe.

    python tools/cross_fp8_probe.py            # prints one JSON line and writes it to profiles/cross_fp8_probe.json
"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("attention", 448), ("attention", 112), ("quantize", 128))
HEADS, KEYS, REPS, SETS = 16, 1500, 30, 2


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
    d, rows = HEADS * 64, windows * HEADS * KEYS
    if kind == "quantize":
        src = [(0.8 * torch.randn((rows, 64), device="cuda")).half() for _ in range(SETS)]
        b, s = torch.empty((rows, 64), dtype=torch.uint8, device="cuda"), torch.empty(rows, dtype=torch.float32, device="cuda")
        us = _median_us({"quantize": lambda i: binding.check(L.wh_op_quantize_kv(None, p(src[i % SETS]), p(b), p(s), rows))})["quantize"]
        return {"quantize_rows": rows, "quantize_us": round(us, 1), "quantize_tbs": round(rows * (128 + 64 + 4) / us / 1e6, 3)}
    K = [(0.8 * torch.randn((windows, HEADS, KEYS, 64), device="cuda")).half() for _ in range(SETS)]
    V = [torch.randn((windows, HEADS, KEYS, 64), device="cuda").half() for _ in range(SETS)]
    q8 = []
    for k, v in zip(K, V):
        set8 = []
        for t in (k, v):
            b, s = torch.empty((rows, 64), dtype=torch.uint8, device="cuda"), torch.empty(rows, dtype=torch.float32, device="cuda")
            binding.check(L.wh_op_quantize_kv(None, p(t), p(b), p(s), rows))
            set8 += [b, s]
        q8.append(set8)
    x = torch.randn((windows, d), device="cuda") * 2 + 0.3
    lw, lb = 1 + 0.1 * torch.randn(d, device="cuda"), 0.1 * torch.randn(d, device="cuda")
    wq, bq = (torch.randn((d, d), device="cuda") / d ** 0.5).half(), 0.1 * torch.randn(d, device="cuda")
    out = torch.zeros((windows, d), device="cuda", dtype=torch.float16)
    scale = C.c_float(64.0 ** -0.25)
    us = _median_us({
        "fp16": lambda i: binding.check(L.wh_op_decoder_cross_attention(None, p(x), p(lw), p(lb), p(wq), p(bq), scale, p(K[i % SETS]), p(V[i % SETS]), p(out), windows, HEADS, KEYS, KEYS, 1)),
        "fp8": lambda i: binding.check(L.wh_op_decoder_cross_attention_f8(None, None, p(x), p(lw), p(lb), p(wq), p(bq), scale, *[p(t) for t in q8[i % SETS]], p(out), windows, HEADS, 1, KEYS, KEYS, 1)),
    })
    n = "w%d" % windows
    return {n + "_fp16_us": round(us["fp16"], 1), n + "_fp16_tbs": round(2.0 * rows * 128 / us["fp16"] / 1e6, 3),
            n + "_fp8_us": round(us["fp8"], 1), n + "_fp8_tbs": round(2.0 * rows * 68 / us["fp8"] / 1e6, 3),
            n + "_time_ratio": round(us["fp8"] / us["fp16"], 3), "byte_ratio": round(68 / 128, 3)}


def main():
    if len(sys.argv) == 3:
        print(json.dumps(step(sys.argv[1], int(sys.argv[2]))))
        return 0
    rec = {"probe": "cross_fp8", "heads": HEADS, "keys": KEYS, "reps": REPS}
    for kind, windows in STEPS:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), kind, str(windows)], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print("step %s %d ended with status %d: nothing more is started" % (kind, windows, r.returncode), file=sys.stderr)
            return 1
        rec.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(rec)
    print(line)
    with open(os.path.join(ROOT, "profiles", "cross_fp8_probe.json"), "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
