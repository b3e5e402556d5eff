"""What constrained decoding costs, on the device.

    python tools/constraint_probe.py [--out profiles/constraint_probe.json] [--launches 30]

mask   wh_op_constraint_mask (constraintMaskKernel, once per wh_context_set_constraint) at the multilingual medium vocabulary (eot 50257) for automata of 64, 1024
       and 4096 states over 16 byte classes -- 4096 x 16 is the 65536-entry limit of the LDS table -- with 10 % of the transitions missing, so that walks are long.
       The vocabulary is random bytes, token lengths 1 .. 12 (mean 6.5) and one token of 255.
apply  wh_op_constraint_apply (constraintApplyKernel, one launch per step) at 1, 32 and 448 rows of 51865 columns, every row on a live state and fed a text
       token. The logits rotate through buffers that together exceed the last-level cache (at most 64 buffers).
step   the same decode step of the device-side loop without and with the launch, at 1, 32 and 448 sequences (steps() below says how).
Device events around every launch of mask and apply, 5 warm-up launches, three medians of --launches launches each. Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EOT, COLS, CLASSES = 50257, 51865, 16


def timed(torch, launches, fn):
    for i in range(5):
        fn(i)
    out = []
    for _ in range(3):
        us = []
        for i in range(launches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(i)
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
        out.append(round(float(np.median(us)), 2))
    return dict(us=out, median_us=round(float(np.median(out)), 2), spread_us=round(max(out) - min(out), 2))


def steps(torch, binding):
    """The same decode step without and with the launch: windows of 64 steps of the d = 128 test model at 1, 32 and 448 sequences, the constraint off and on,
    alternating, 7 timed windows each behind one that captures; host clock from the enqueue to the window's end over the 65 samples. The constraint forbids every
    odd-numbered token (one invented byte per token) at a penalty of 1e-30: every row pays the walk, the line and the stores, and no float changes enough to
    change a token, so both sides decode the same window."""
    import time
    from whisper_amd import ggml_format as gf
    hp = gf.hparams_for("test-d128-ml")
    model = binding.HipModel.from_ggml(gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=4))
    sp, n_steps, out = gf.special_tokens(hp), 64, {}
    eot = sp["eot"]
    dfa = dict(class_of=np.arange(256) & 1, trans=np.array([[0, -1]], np.int32), accept=np.ones(1, np.uint8), start=0,
               tok_offsets=np.arange(eot + 1, dtype=np.int32), tok_bytes=(np.arange(eot) & 255).astype(np.uint8), penalty=1e-30)
    rng = np.random.default_rng(17)
    for batch in (1, 32, 448):
        ctx = binding.HipContext(model, batch)
        ctx.encode(torch.from_numpy(rng.uniform(-1, 1, (batch, 80, 3000)).astype(np.float32)).cuda())
        prompt = np.array([[sp["prev"], 1000 + b % 64, sp["sot"], sp["sot"] + 1] for b in range(batch)], np.int32)
        times, ids = {False: [], True: []}, {}
        for rep in range(8):
            for on in (False, True):
                ctx.set_constraint(**dfa) if on else ctx.set_constraint()
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.decode_window_start(prompt, n_steps)
                data = ctx.decode_window_fetch_data(0, 1 + n_steps)
                ctx.decode_window_finish()
                if rep:                                                          # the first round captures
                    times[on].append((time.perf_counter() - t0) / (1 + n_steps) * 1e6)
                ids[on] = data["id"]
        assert np.array_equal(ids[False], ids[True]), "the probe's constraint must not change the window"
        off, on = (float(np.median(times[k])) for k in (False, True))
        out["%d_rows" % batch] = dict(off_us=round(off, 1), on_us=round(on, 1), added_us=round(on - off, 1),
                                      spread_off_us=round(max(times[False]) - min(times[False]), 1), spread_on_us=round(max(times[True]) - min(times[True]), 1))
        ctx.close()
    model.close()
    return dict(model="test-d128-ml", steps=n_steps, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=30)
    a = ap.parse_args()
    import torch
    from whisper_amd import binding
    L = binding.lib()
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 13, EOT)
    lens[1234] = 255
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    data = rng.integers(0, 256, int(offsets[-1]) + 1).astype(np.uint8)
    class_of = rng.integers(0, CLASSES, 256).astype(np.uint8)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()             # noqa: E731
    d_off, d_data, d_cls = dev(offsets), dev(data), dev(class_of)
    words = (EOT + 31) // 32
    res = dict(eot=EOT, cols=COLS, classes=CLASSES, launches=a.launches, mask={}, apply={})
    for n_states in (64, 1024, 4096):
        trans = rng.integers(0, n_states, (n_states, CLASSES)).astype(np.int32)
        trans[rng.random(trans.shape) < 0.1] = -1
        d_trans, d_acc = dev(trans), dev(np.ones(n_states, np.uint8))
        allowed = torch.zeros(n_states * words, dtype=torch.int32, device="cuda")
        t = binding.ConstraintTablesC(n_states, CLASSES, 0, EOT, d_cls.data_ptr(), d_trans.data_ptr(), d_acc.data_ptr(), d_off.data_ptr(), d_data.data_ptr(), int(offsets[-1]))
        res["mask"]["%d_states" % n_states] = timed(torch, a.launches, lambda i: binding.check(L.wh_op_constraint_mask(None, C.byref(t), C.c_void_p(allowed.data_ptr()))))
        if n_states != 1024:
            continue
        for rows in (1, 32, 448):
            n_buf = min(64, max(2, int(600e6 // (rows * COLS * 4)) + 1))
            bufs = [torch.randn(rows, COLS, device="cuda") for _ in range(n_buf)]
            states = dev(rng.integers(0, n_states, rows).astype(np.int32))
            fed = dev(rng.integers(0, EOT, rows).astype(np.int32))
            keep = states.clone()

            def step(i):
                states.copy_(keep)
                binding.check(L.wh_op_constraint_apply(None, C.c_void_p(bufs[i % n_buf].data_ptr()), rows, COLS, EOT, C.byref(t), C.c_void_p(allowed.data_ptr()),
                                                       C.c_void_p(states.data_ptr()), C.c_void_p(fed.data_ptr()), 0, 100.0))

            r = timed(torch, a.launches, step)
            r["note"] = "includes one %d-byte device copy that puts the states back" % (4 * rows)
            res["apply"]["%d_rows" % rows] = r
            del bufs
    res["step"] = steps(torch, binding)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
