"""Language detection's kernel against the composition it replaces, on the device.

    python tools/lang_detect_probe.py [--out profiles/lang_detect_probe.json] [--launches 30]

langProbsKernel (wh_op_lang_probs: one read of the logits, 99 probabilities and one index written per row) against
wh_op_vocab_soft_max followed by a device gather + argmax of the language columns (the full row of probabilities written and read
back), at 64 and 448 rows of 51865 logits. hip-event time per launch, warm-up first, median of --launches launches; the inputs rotate
through buffers that together exceed the last-level cache (512 MB), so that no launch finds its row there. --prepass 448 adds the wall time of the detection pre-pass of a 448-stream lock-step batch (encoder batch + detection
step, ggml-medium shape) next to one ordinary round of that batch. Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLS, SOT, N_LANG = 51865, 50258, 99
ROTATE_BYTES = 512 << 20


def ptr(t):
    return C.c_void_p(t.data_ptr())


def timed(torch, fn, bufs, launches, warmup=5):
    for i in range(warmup):
        fn(bufs[i % len(bufs)])
    torch.cuda.synchronize()
    ms = []
    for i in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(bufs[(warmup + i) % len(bufs)])
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)) * 1e3


def prepass(torch, binding, streams, steps=28, repeats=5):
    """Wall time of the detection pre-pass of a lock-step batch of `streams` first windows on one context of the ggml-medium shape (random weights):
    wh_encode_windows + wh_lang_detect, next to ONE ordinary round of the same batch (wh_encode_windows + a 3-token prompt step + `steps` greedy steps,
    the shape of the headline bench's round) and to the detection step alone. Median of `repeats` after one warm-up."""
    import time
    import bench
    from whisper_amd import ggml_format as gf
    model = gf.synth_model("medium", seed=1)
    sp = gf.special_tokens(model.hparams)
    m = binding.HipModel.from_ggml(model)
    del model
    ctx = binding.HipContext(m, streams)
    pcm = torch.from_numpy(bench.synth_pcm(7, seed=100)).cuda()
    mels = ctx.mel_spectrogram_batch(pcm)
    wins = [(mels[i % 7], 0) for i in range(streams)]
    prompt = np.asarray([[sp["sot"], sp["sot"] + 1, sp["transcribe"]]] * streams, np.int32)

    def wall(fn):
        t = []
        for i in range(repeats + 1):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            t.append(time.perf_counter() - t0)
        return float(np.median(t[1:])) * 1e3

    def detect():
        ctx.encode_windows(wins)
        ctx.lang_detect()

    def round_():
        ctx.encode_windows(wins)
        ctx.decode_window_start(prompt, steps)
        ctx.decode_window_finish()

    out = dict(streams=streams, greedy_steps=steps, encode_ms=wall(lambda: ctx.encode_windows(wins)), prepass_ms=wall(detect), round_ms=wall(round_))
    ctx.encode_windows(wins)
    out["detect_step_ms"] = wall(lambda: ctx.lang_detect())
    ctx.close()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--prepass", type=int, default=0, metavar="STREAMS", help="also time the detection pre-pass of a lock-step batch of STREAMS windows (ggml-medium shape)")
    a = ap.parse_args()
    import torch
    from whisper_amd import binding
    L = binding.lib()
    res = dict(cols=COLS, n_lang=N_LANG, launches=a.launches, rows={})
    for rows in (64, 448):
        row_bytes = rows * COLS * 4
        n_buf = ROTATE_BYTES // row_bytes + 2
        g = torch.Generator(device="cuda").manual_seed(rows)
        bufs = [3.0 * torch.randn((rows, COLS), generator=g, device="cuda", dtype=torch.float32) for _ in range(n_buf)]
        probs = torch.empty((rows, COLS), dtype=torch.float32, device="cuda")
        lang_p = torch.empty((rows, N_LANG), dtype=torch.float32, device="cuda")
        best = torch.empty((rows,), dtype=torch.int32, device="cuda")

        def fused(x):
            binding.check(L.wh_op_lang_probs(None, ptr(x), rows, COLS, SOT, N_LANG, ptr(lang_p), ptr(best)))

        def composition(x):
            binding.check(L.wh_op_vocab_soft_max(None, ptr(x), ptr(probs), rows, COLS))
            blk = probs[:, SOT + 1:SOT + 1 + N_LANG].contiguous()
            torch.argmax(blk, dim=1)

        def soft_max_only(x):
            binding.check(L.wh_op_vocab_soft_max(None, ptr(x), ptr(probs), rows, COLS))

        r = dict(buffers=n_buf, fused_us=timed(torch, fused, bufs, a.launches), composition_us=timed(torch, composition, bufs, a.launches),
                 soft_max_only_us=timed(torch, soft_max_only, bufs, a.launches))
        # the same result from both
        composition(bufs[0])
        fused(bufs[0])
        torch.cuda.synchronize()
        assert torch.equal(lang_p, probs[:, SOT + 1:SOT + 1 + N_LANG]) and torch.equal(best.long(), torch.argmax(probs[:, SOT + 1:SOT + 1 + N_LANG], dim=1))
        r["fused_gb_s"] = row_bytes / r["fused_us"] * 1e-3
        res["rows"][str(rows)] = r
        del bufs
        torch.cuda.empty_cache()
    if a.prepass:
        res["prepass"] = prepass(torch, binding, a.prepass)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
