"""What token alignment (eFullParamsFlags::AlignTokens, wh_align_tokens) costs on the device.

    python tools/align_probe.py [--out profiles/align_probe.json] [--kind medium] [--launches 30]

At the shape of --kind (default: ggml-medium, 24 decoder layers x 16 heads, the default selection = 192 heads), for windows of 54 rows (49 text tokens, what the
single-stream workload of bench.py transcribes per window) and of 228 rows (the longest a window can be), all 1500 keys:
  matrix_us / dtw_us   hip-event time of wh_op_align_matrix (both sweeps) and wh_op_dtw on seeded FP16 q / k, warm-up first, median of --launches launches;
  total_ms             host wall time of wh_align_tokens (upload, the decoder pass to the last selected layer, matrix, DTW, frames back), median of --launches;
  pass_ms              total_ms - matrix - dtw: the teacher-forced decoder pass and the host round trip, derived, not measured on its own.
Then iContext::runFull through libWhisper.so on the scripted single-stream workload of bench.py (7 windows of 51 tokens over 198.762 s of audio, prompt carry-over
capped at 102 tokens) with and without the flag, alternating, best of --runs each: audio-seconds per second. Prints one JSON line."""
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

CLIP_SECONDS = 198.762


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--kind", default="medium")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    import torch
    from whisper_amd import api, binding, ggml_format as gf
    if not torch.cuda.is_available():
        raise SystemExit("align_probe: no GPU")
    L = binding.lib()
    hp = gf.hparams_for(a.kind)
    sp = gf.special_tokens(hp)
    H, d, T = hp.n_text_head, hp.n_text_state, hp.n_audio_ctx
    layer0 = hp.n_text_layer // 2
    heads = [(l, h) for l in range(layer0, hp.n_text_layer) for h in range(H)]
    res = dict(kind=a.kind, launches=a.launches, heads=len(heads), keys=T, windows={})
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def event_us(launch):
        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(us)), float(np.min(us)), float(np.max(us))

    # ---- the kernels alone, on seeded operands ----
    g = torch.Generator(device="cuda").manual_seed(1)
    k = (0.5 * torch.randn((hp.n_text_layer, 1, H, T, 64), generator=g, device="cuda")).half()
    heads_d = torch.tensor(heads, dtype=torch.int32, device="cuda")
    keys_d = torch.tensor([T], dtype=torch.int32, device="cuda")
    for rows in (54, 228):
        q = (0.5 * torch.randn((hp.n_text_layer - layer0, 1, rows, d), generator=g, device="cuda")).half()
        rows_d = torch.tensor([rows], dtype=torch.int32, device="cuda")
        stats = torch.empty((1, len(heads), rows, 2), dtype=torch.float32, device="cuda")
        M = torch.empty((1, rows, T), dtype=torch.float32, device="cuda")
        frames = torch.empty((1, rows), dtype=torch.int32, device="cuda")

        def matrix():
            binding.check(L.wh_op_align_matrix(stream, C.c_void_p(q.data_ptr()), rows * d, layer0, C.c_void_p(k.data_ptr()), H * T * 64, hp.n_text_layer, H, T,
                                               C.c_void_p(heads_d.data_ptr()), len(heads), C.c_void_p(rows_d.data_ptr()), C.c_void_p(keys_d.data_ptr()), 1, rows, T,
                                               C.c_void_p(stats.data_ptr()), C.c_void_p(M.data_ptr())))

        def dtw():
            binding.check(L.wh_op_dtw(stream, C.c_void_p(M.data_ptr()), 1, rows, T, C.c_void_p(rows_d.data_ptr()), C.c_void_p(keys_d.data_ptr()), C.c_void_p(frames.data_ptr())))

        m_us = event_us(matrix)
        d_us = event_us(dtw)
        # algorithmic work of the matrix: S twice in sweep 1 and once (with the halo, 32 / 26) in sweep 2, 2 x 64 flop per score; the K rows of the selected layers
        flops = len(heads) * rows * T * 128.0 * (2 + 32.0 / 26.0)
        res["windows"]["%d_rows" % rows] = dict(rows=rows, matrix_us=m_us[0], matrix_us_min=m_us[1], matrix_us_max=m_us[2], dtw_us=d_us[0], dtw_us_min=d_us[1],
                                                dtw_us_max=d_us[2], matrix_tflops=flops / m_us[0] * 1e-6, k_mb=len(heads) * T * 64 * 2 / 1e6)
    del k
    torch.cuda.empty_cache()

    # ---- wh_align_tokens end to end on a random-weight model of the shape ----
    model = gf.synth_model(a.kind, seed=1)
    hm = binding.HipModel.from_ggml(model)
    ctx = binding.HipContext(hm, 1)
    rng = np.random.default_rng(3)
    pcm = (0.1 * rng.standard_normal(30 * 16000)).astype(np.float32)
    ctx.encode(ctx.mel_spectrogram(torch.from_numpy(pcm).cuda()))
    for rows in (54, 228):
        n_text = rows - 5 if hp.n_vocab >= 51865 else rows - 3
        sot = [sp["sot"], sp["sot"] + 1, sp["transcribe"]] if hp.n_vocab >= 51865 else [sp["sot"]]
        row = sot + [sp["not_"]] + [int(x) for x in rng.integers(1000, 40000, n_text)] + [sp["eot"]]
        for _ in range(3):
            ctx.align_tokens([row], [T])
        wall = []
        for _ in range(a.launches):
            t0 = time.perf_counter()
            ctx.align_tokens([row], [T])
            wall.append(time.perf_counter() - t0)
        w = res["windows"]["%d_rows" % rows]
        w["total_ms"] = float(np.median(wall)) * 1e3
        w["pass_ms_derived"] = w["total_ms"] - (w["matrix_us"] + w["dtw_us"]) * 1e-3
    ctx.close()
    hm.close()
    del model

    # ---- runFull with and without the flag: the single-stream workload of bench.py ----
    cap = 102
    positions, kept = gf.carry_over_script(hp, 7, 49, cap)
    scripted = gf.scripted_model_at(positions, kind=a.kind, seed=7)
    clip = (0.05 * np.random.default_rng(100).standard_normal(int(CLIP_SECONDS * 16000))).astype(np.float32)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "scripted.bin")
        gf.write_model(path, scripted)
        del scripted
        m = api.Model(path)
        c = m.create_context()
        best = {0: 1e9, api.ALIGN_TOKENS: 1e9}
        tokens = {}
        for flags in best:
            c.run_full(clip, n_max_text_ctx=cap, flags=flags)          # warm-up: graph capture, first-use buffers
            tokens[flags] = [t["id"] for s in c.results() for t in s["tokens"]]
        for _ in range(a.runs):
            for flags in best:
                t0 = time.perf_counter()
                c.run_full(clip, n_max_text_ctx=cap, flags=flags)
                best[flags] = min(best[flags], time.perf_counter() - t0)
                tokens[flags] = [t["id"] for s in c.results() for t in s["tokens"]]          # steady state: every run starts from the previous run's carried-over prompt
        aligned = sum(1 for s in c.results() for t in s["tokens"] if t["t1"] > t["t0"])
        res["run_full"] = dict(clip_seconds=CLIP_SECONDS, windows=7, tokens=len(tokens[0]), same_tokens=tokens[0] == tokens[api.ALIGN_TOKENS], tokens_with_a_duration=aligned,
                               audio_s_per_s=CLIP_SECONDS / best[0], audio_s_per_s_align=CLIP_SECONDS / best[api.ALIGN_TOKENS],
                               seconds=best[0], seconds_align=best[api.ALIGN_TOKENS], ms_per_window_added=(best[api.ALIGN_TOKENS] - best[0]) / 7 * 1e3, runs=a.runs)
        c.close()
        m.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
