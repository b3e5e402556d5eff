"""Generates tests/golden/ref_lang_detect.json: what the reference's CPU model answers when the language is left to it --
whisper_lang_auto_detect (Whisper/source/whisper.cpp:2428-2495) and the "auto" branch of whisper_full (:2788-2801) -- on models
whose language token is decided by the audio and reaches the transcript (whisper_amd.ggml_format.language_conditioned_model).

Run in the build container: make -C oracle && python tests/golden/make_golden_lang_detect.py

Same recordings, model kind, prompt and n_max_text_ctx as make_golden_runfull.py. A (seed, recording) pair is kept only if the reference
at 1, 4 and 8 threads names the same winner and gives the same transcript, and if both the top-1 / top-2 logit margin inside the language
block and the smallest margin along the transcript are at least MIN_MARGIN (make_golden_runfull.py's constant for audio-conditioned
cases). The conditions on the SET of cases are asserted in main(): no test can hide a failure by shedding cases."""
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from whisper_amd import ggml_format as gf  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden_runfull import KIND, MIN_MARGIN, PROMPT_LEN, pcm_for  # noqa: E402

SELF_OUT_SCALE = 20.0                           # decoder layer 0's attn.out: large enough for the language token to move the transcript, small enough for thread-stable cases
# (seed, recording) pairs, chosen like make_golden_runfull.py's seeds: seeds 10 .. 29 were looked at (about one pair in three passes every condition below;
# the longer recordings mostly fail the transcript margin); three pairs that are rejected stay in the list as a record of why pairs are
PAIRS = [(10, "jfk"), (10, "mixed"), (11, "jfk"), (11, "mixed"), (12, "jfk"), (13, "jfk"), (16, "jfk"), (17, "jfk"), (18, "jfk"), (24, "jfk"), (25, "jfk"),
         (27, "jfk"), (28, "jfk"), (29, "jfk")]
MAX_TRIED, MIN_KEPT, MIN_WINNERS, MIN_SENSITIVE = 24, 8, 3, 3
OUT = os.path.join(HERE, "ref_lang_detect.json")
LANG_CODES = ("en", "zh", "de", "es", "ru", "ko", "fr")       # ids 0 .. 6 of the reference's table (whisper.cpp:31-133)


def model_for(seed: int):
    hp = gf.hparams_for(KIND)
    return gf.language_conditioned_model(gf.conditioned_layout(hp), PROMPT_LEN, kind=KIND, seed=seed, self_out_scale=SELF_OUT_SCALE)


def ref_lang_lib():
    """The detection entry points libwhisper_ref.so exports and oracle/ref.py does not wrap."""
    from oracle import ref
    L = ref.lib()
    L.whisper_lang_auto_detect.restype = C.c_int
    L.whisper_lang_auto_detect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.whisper_lang_max_id.restype = C.c_int
    L.whisper_lang_str.restype = C.c_char_p
    L.whisper_lang_str.argtypes = [C.c_int]
    return L


def bits(a):
    return [int(v) for v in np.ascontiguousarray(a, np.float32).view(np.uint32)]


def from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def detect(w, offset_ms: int = 0):
    """whisper_lang_auto_detect on the spectrogram the context holds: (return code or winner id, p on the language tokens = ctx->probs there,
    lang_probs, logits of the language block)."""
    L = ref_lang_lib()
    n_lang = L.whisper_lang_max_id() + 1
    probs = np.zeros(n_lang, np.float32)
    rc = L.whisper_lang_auto_detect(w.ctx, offset_ms, w.n_threads, probs.ctypes.data_as(C.c_void_p))
    if rc < 0:
        return rc, None, None, None
    n = w.L.ref_logits_size(w.ctx)
    logits, p = np.zeros(n, np.float32), np.zeros(n, np.float32)
    w.L.ref_get_logits(w.ctx, logits)
    w.L.ref_get_probs(w.ctx, p)
    sot = 50258                                   # multilingual vocabularies (51865 and the large-v3 shape's 51866)
    blk = slice(sot + 1, sot + 1 + (w.n_vocab - 51766))
    return rc, p[-w.n_vocab:][blk].copy(), probs, logits[-w.n_vocab:][blk].copy()


def full(w, pcm, lang):
    segs = w.full(pcm, lang=lang, no_context=True, prompt=[1000], n_max_text_ctx=0)
    return [dict(t0=s["t0"], t1=s["t1"], text=s["text"].decode(), tokens=s["tokens"], probs=[round(float(p), 5) for p in s["probs"]]) for s in segs]


def strip(r):
    return [(s["t0"], s["t1"], s["tokens"]) for s in r]


def replay_margins(w, pcm, sp, lang_id, want_tokens):
    """make_golden_runfull.replay_margins with the language token of the prompt given: the smallest top-1 / top-2 logit margin along the
    transcript, through whisper_decode step by step; asserts that the replay chooses whisper_full's tokens."""
    w.pcm_to_mel(pcm)
    n_frames = len(pcm) // 160
    seek, got, margin = 0, [], 1e9
    prompt = [sp["prev"], sp["sot"], sp["sot"] + 1 + lang_id, sp["transcribe"]]
    while seek + 100 < n_frames:
        w.encode(seek)
        # whisper_full drops the past prompt -- here: the [prev] token -- when less than 5 s remain (whisper.cpp:2874-2878)
        toks, n_past, delta, cur = list(prompt[1:] if seek > 0 and seek + 500 >= n_frames else prompt), 0, 3000, []
        has_ts = False
        for i in range(220):
            logits, _ = w.decode(toks, n_past)
            sb = w.sample_timestamp(True) if i == 0 else w.sample_best()
            top = np.sort(logits[-1][sp["beg"]:] if sb["id"] >= sp["beg"] else logits[-1])[-2:]
            margin = min(margin, float(top[1] - top[0]))
            n_past += len(toks)
            toks = [sb["id"]]
            if sb["id"] == sp["eot"]:
                break
            cur.append(sb["id"])
            if sb["id"] > sp["beg"]:
                delta, has_ts = 2 * (sb["id"] - sp["beg"]), True
            if has_ts and seek + delta + 100 >= n_frames:      # the end of the audio ends the window (whisper.cpp:2967-2970)
                break
        got += cur
        seek += delta
    text = lambda ids: [t for t in ids if t < sp["eot"]]
    assert text(got) == text(want_tokens), (got, want_tokens)
    return margin


def make_case(seed: int, rec: str, verbose: bool = True):
    """The record of one (seed, recording) pair, or (None, reason) when the reference's own thread count decides something."""
    from oracle import ref
    pcm = pcm_for(rec)
    sp = gf.special_tokens(gf.hparams_for(KIND))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "m.bin")
        gf.write_model(path, model_for(seed))
        det, res = {}, {}
        for nt in (1, 4, 8):
            w = ref.RefWhisper(path, n_threads=nt, log_level=0)
            w.pcm_to_mel(pcm)
            det[nt] = detect(w)
            res[nt] = full(w, pcm, "auto")
            w.close()
        winner = det[4][0]
        if not (det[1][0] == det[4][0] == det[8][0]):
            return None, "the winner depends on the reference's thread count"
        if not (strip(res[1]) == strip(res[4]) == strip(res[8])):
            return None, "the transcript depends on the reference's thread count"
        top = np.sort(det[4][3])[-2:]
        lang_margin = float(top[1] - top[0])
        if lang_margin < MIN_MARGIN:
            return None, "language margin %.4f" % lang_margin
        w = ref.RefWhisper(path, n_threads=4, log_level=0)
        try:
            margin = replay_margins(w, pcm, sp, winner, [t for s in res[4] for t in s["tokens"]])
        except AssertionError:
            w.close()
            return None, "a window of this transcript takes a rule the step-by-step replay does not restate: no margin to be had"
        if margin < MIN_MARGIN:
            w.close()
            return None, "transcript margin %.4f" % margin
        named = full(w, pcm, LANG_CODES[winner])
        assert strip(named) == strip(res[4]), "whisper_full( auto ) differs from whisper_full( winner )"
        differs = [LANG_CODES[lid] for lid in gf.LANGUAGE_CANDIDATES if lid != winner and strip(full(w, pcm, LANG_CODES[lid])) != strip(res[4])]
        w.close()
    p_spread = float(max(np.abs(det[1][1] - det[4][1]).max(), np.abs(det[8][1] - det[4][1]).max()))
    rec_out = dict(name="%s_s%d" % (rec, seed), pcm=rec, seed=seed, n_samples=len(pcm), prompt=[1000], n_max_text_ctx=0,
                   winner=LANG_CODES[winner], winner_id=int(winner), p_bits=bits(det[4][1]), lang_probs_bits=bits(det[4][2]),
                   lang_logit_margin=round(lang_margin, 4), min_logit_margin=round(margin, 4), p_spread=p_spread,
                   transcript_differs_under=differs, segments=res[4])
    if verbose:
        print("    winner %s p %.3f -> lang_probs %.4f, language margin %.3f, transcript margin %.3f, p_spread %.2e, transcript differs under %s" %
              (LANG_CODES[winner], det[4][1][winner], det[4][2][winner], lang_margin, margin, p_spread, differs))
    return rec_out, ""


# The frame-0 rule: whisper_full detects at offset 0 WHATEVER params.offset_ms is (whisper.cpp:2792). A recording whose language token at 15 s is another
# one than at frame 0, so that a run with offset_ms = 15000 tells the two rules apart (seeds 10 .. 20 x the three longer recordings were looked at).
OFFSET_PAIR, OFFSET_MS = (10, "quiet"), 15000


def full_range(w, pcm, lang, offset_ms):
    rc, segs = w.full_range(pcm, lang=lang, flags=1, prompt=[1000], n_max_text_ctx=0, offset_ms=offset_ms)
    assert rc == 0, rc
    return [dict(t0=s["t0"], t1=s["t1"], text=s["text"], tokens=s["tokens"]) for s in segs]


def make_offset_case():
    """whisper_full( "auto", offset_ms = OFFSET_MS ) on OFFSET_PAIR: asserts that 1, 4 and 8 reference threads agree on the winner at frame 0, on the winner a
    detection AT the offset would name, and on the transcript; that the two winners differ, both by at least MIN_MARGIN logits; and that the run's
    transcript is the one of the frame-0 winner named."""
    from oracle import ref
    seed, rec = OFFSET_PAIR
    pcm = pcm_for(rec)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "m.bin")
        gf.write_model(path, model_for(seed))
        d0, d1, res = {}, {}, {}
        for nt in (1, 4, 8):
            w = ref.RefWhisper(path, n_threads=nt, log_level=0)
            w.pcm_to_mel(pcm)
            d0[nt], d1[nt] = detect(w, 0), detect(w, OFFSET_MS)
            res[nt] = full_range(w, pcm, "auto", OFFSET_MS)
            w.close()
        assert d0[1][0] == d0[4][0] == d0[8][0] and d1[1][0] == d1[4][0] == d1[8][0], "a winner depends on the reference's thread count"
        assert d0[4][0] != d1[4][0], "the language at the offset is the language at frame 0: this pair cannot tell the rules apart"
        m0, m1 = np.sort(d0[4][3])[-2:], np.sort(d1[4][3])[-2:]
        assert m0[1] - m0[0] >= MIN_MARGIN and m1[1] - m1[0] >= MIN_MARGIN
        assert strip(res[1]) == strip(res[4]) == strip(res[8]) and len(res[4]) > 0, "the transcript depends on the reference's thread count"
        w = ref.RefWhisper(path, n_threads=4, log_level=0)
        assert strip(full_range(w, pcm, LANG_CODES[d0[4][0]], OFFSET_MS)) == strip(res[4])
        differs = strip(full_range(w, pcm, LANG_CODES[d1[4][0]], OFFSET_MS)) != strip(res[4])
        w.close()
    return dict(name="%s_s%d_offset" % (rec, seed), pcm=rec, seed=seed, n_samples=len(pcm), prompt=[1000], n_max_text_ctx=0, offset_ms=OFFSET_MS,
                winner=LANG_CODES[d0[4][0]], winner_id=int(d0[4][0]), winner_at_offset=LANG_CODES[d1[4][0]], lang_logit_margin=round(float(m0[1] - m0[0]), 4),
                lang_logit_margin_at_offset=round(float(m1[1] - m1[0]), 4), transcript_differs_under_the_language_at_the_offset=bool(differs), segments=res[4])


def main():
    if "--offset-only" in sys.argv:                                   # re-make the offset case alone, the other cases as committed
        with open(OUT) as f:
            fx = json.load(f)
        fx["offset_case"] = make_offset_case()
        with open(OUT, "w") as f:
            json.dump(fx, f, indent=1)
        print(fx["offset_case"])
        return
    out, tried = [], 0
    for seed, rec in PAIRS[:MAX_TRIED]:
        tried += 1
        c, why = make_case(seed, rec)
        print("seed", seed, rec, "->", "kept" if c else "REJECTED: " + why)
        if c:
            out.append(c)
    assert tried <= MAX_TRIED and len(out) >= MIN_KEPT, (tried, len(out))
    assert len({c["winner"] for c in out}) >= MIN_WINNERS, sorted({c["winner"] for c in out})
    assert sum(1 for c in out if c["transcript_differs_under"]) >= MIN_SENSITIVE
    with open(OUT, "w") as f:
        json.dump(dict(kind=KIND, prompt_len=PROMPT_LEN, self_out_scale=SELF_OUT_SCALE, min_margin=MIN_MARGIN, cases=out, offset_case=make_offset_case()), f, indent=1)
    print("%d of %d kept, winners %s, largest p_spread %.3e" % (len(out), tried, sorted({c["winner"] for c in out}), max(c["p_spread"] for c in out)))


if __name__ == "__main__":
    main()
