"""Writes tests/golden/ref_score_d128.json: the yardstick of tests/test_gpu_score.py, computed on the CPU by the two oracles of oracle/whisper_np.py.

A conditioned model (test-d128-ml, 36 scripted positions behind a 4-token prompt) and three windows of seeded audio. Row b is the prompt followed by the
greedy transcript of WhisperTruth (float64, teacher forced), cut to LENS[b] tokens; entries FIRST[b] .. LENS[b] - 1 are scored. Per scored entry: the record of
tests/token_score_ref.py on WhisperTruth's row, truth's margin between its two best ids and between the target and the id nearest to it in value, and the
log-probability WhisperNP's row (the reference's numerics, FP32 P.V) gives. `bad` is window 2's row with every third text token replaced.

    python tests/golden/make_golden_score.py            (about 10 s)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from oracle import whisper_np as wn  # noqa: E402
from whisper_amd import ggml_format as gf  # noqa: E402
import token_score_ref as TS  # noqa: E402

MODEL_SEED, MEL_SEED = 10, 17
LENS, FIRST = (5, 12, 40), (4, 6, 5)
PROMPT_LEN = 4


def layout(sp):
    return [("ts", (0, 40))] + [("text", None)] * 33 + [("ts", (700, 1100)), ("tok", sp["eot"])]


def model():
    hp = gf.hparams_for("test-d128-ml")
    return gf.conditioned_model(layout(gf.special_tokens(hp)), PROMPT_LEN, kind="test-d128-ml", seed=MODEL_SEED)


def mels():
    return np.random.default_rng(MEL_SEED).uniform(-1, 1, (len(LENS), 80, 3000)).astype(np.float32)


def corrupted(row, first):
    """Every third text token from `first` on replaced by another text token (the closing timestamp and eot stay)"""
    bad = list(row)
    for i in range(first, len(row) - 2, 3):
        bad[i] = row[i] + 7
    return bad


def entries(truth_rows, np_rows, row, first):
    out = []
    for i in range(first, len(row)):
        x = truth_rows[i - 1]
        lp, blp, best, rank = TS.score_row(x, row[i])
        srt = np.sort(x)
        out.append(dict(i=i, token=int(row[i]), logprob=lp, bestLogprob=blp, best=best, rank=rank, top2_margin=float(srt[-1] - srt[-2]),
                        target_margin=float(np.abs(np.delete(x, row[i]) - x[row[i]]).min()), np_logprob=TS.score_row(np_rows[i - 1], row[i])[0],
                        np_best=TS.score_row(np_rows[i - 1], row[i])[2], np_rank=TS.score_row(np_rows[i - 1], row[i])[3]))
    return out


def main():
    ggml = model()
    sp = gf.special_tokens(ggml.hparams)
    m = mels()
    npm, tr = wn.WhisperNP(ggml), wn.WhisperTruth(ggml)
    windows, dev = [], 0.0
    for b, n in enumerate(LENS):
        npm.encode(m[b])
        tr.encode(m[b].astype(np.float64))
        row = [sp["prev"], 1000 + b, sp["sot"], sp["sot"] + 1]
        while len(row) < n:
            row.append(int(np.argmax(tr.decode(row, 0)[-1])))
        tl = tr.decode(row, 0)
        nl, _ = npm.decode(row, 0, exact_pv=False)
        dev = max(dev, float(np.abs(nl.astype(np.float64) - tl).max()))
        w = dict(row=row, first=FIRST[b], entries=entries(tl, nl, row, FIRST[b]))
        if b == len(LENS) - 1:
            bad = corrupted(row, FIRST[b])
            w["bad"] = bad
            nb, _ = npm.decode(bad, 0, exact_pv=False)
            w["bad_entries"] = entries(tr.decode(bad, 0), nb, bad, FIRST[b])
        windows.append(w)
    e = [x for w in windows for x in w["entries"]]
    d = np.array([abs(x["np_logprob"] - x["logprob"]) for x in e])
    miss = sum(1 for x in e if (x["np_best"], x["np_rank"]) != (x["best"], x["rank"]))
    out = dict(model_seed=MODEL_SEED, mel_seed=MEL_SEED, np_logit_dev_max=dev, np_logprob_dist_max=float(d.max()), np_logprob_dist_mean=float(d.mean()),
               np_rank_or_best_differs=miss, windows=windows)
    print("WhisperNP against WhisperTruth: largest logit deviation %.3e, |logprob| distance max %.3e mean %.3e, rank / best differ in %d of %d entries" %
          (dev, d.max(), d.mean(), miss, len(e)))
    with open(os.path.join(HERE, "ref_score_d128.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
