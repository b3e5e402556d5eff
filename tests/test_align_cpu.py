"""CPU tests of token alignment: the numpy restatement of the definition (tests/align_ref.py) on hand-worked cases, and the host loop's half --
whisper_amd/host/hostLoop.h with a scripted aligner (tests/align_cpu/driver.cpp): frames -> token times, once per window, never without the flag."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import align_ref as ar  # noqa: E402

BUILD = os.path.join(ROOT, "tests", "_build")
HIP_DIR = os.path.join(ROOT, "whisper_amd", "lib")
DRIVER = os.path.join(BUILD, "align_driver")
SOURCES = [os.path.join(ROOT, "tests", "align_cpu", "driver.cpp")] + [os.path.join(ROOT, "whisper_amd", "host", f) for f in ("support.cpp", "tokenTimestamps.cpp")]
HEADERS = [os.path.join(ROOT, "whisper_amd", "host", f) for f in ("hostLoop.h", "hostCommon.h")] + [os.path.join(ROOT, "include", "whisperApi.h")]

ALIGN_TOKENS, TOKEN_TIMESTAMPS, NO_CONTEXT = 0x1000, 0x100, 2
EOT, SOT, NOT, BEG = 50257, 50258, 50363, 50364          # the multilingual vocabulary of 51865 tokens
SOLM = 50362
EN, TRANSCRIBE = SOT + 1, 50359


# ---------------------------------------------------------------------------------------------------------------------
# align_ref
# ---------------------------------------------------------------------------------------------------------------------
def test_dtw_on_a_hand_worked_matrix():
    """3 x 4 costs whose cheapest monotone path is known: (0,0) (0,1) (1,2) (2,3).
         cost table (row 0 / column 0 = the +inf border, cost[0][0] = 0):
           1  1+3=4   4+9=13  13+9=22
           10 1+9=10  1+4... the path collects 1 + 3 + 1 + 1 = 6."""
    x = np.asarray([[1, 3, 9, 9],
                    [9, 9, 1, 9],
                    [9, 9, 9, 1]], np.float32)
    frames, path = ar.dtw(x)
    assert path == [(0, 0), (0, 1), (1, 2), (2, 3)]
    assert frames.tolist() == [0, 2, 3]
    assert ar.dtw_fast(x).tolist() == [0, 2, 3]


def test_dtw_trace_rule_on_exact_ties():
    """All-zero costs: every cell ties three ways, the rule's last branch (2 = stay in the row, one key back) wins wherever neither strict test holds.
    cost is 0 on the whole table but the +inf border, so: inside, c0 == c1 == c2 -> 2; in row 1 (c0 and c1 from the border row: +inf but for
    cost[0][0]) cell (1,1) has c0 = 0 < inf, inf -> 0. Walking back from (R, N): along row R to column 1 (all 2), then (R,1): c0 = inf (border
    column), c1 = 0, c2 = inf -> 1, up column 1 to (1,1) -> 0. Every row but the last therefore sits on key 0, the last row starts at key 0 too."""
    x = np.zeros((4, 6), np.float32)
    frames, path = ar.dtw(x)
    assert frames.tolist() == [0, 0, 0, 0]
    assert path == [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (3, 2), (3, 3), (3, 4), (3, 5)]
    # integer costs where the diagonal and the row above tie BELOW the cell to the left: neither strict test holds, so the rule still answers 2.
    #   cost table        trace
    #   0  5 10           0 2 2
    #   0  0  5           1 2 2      (2,2): c0 = 0, c1 = 5, c2 = 0 -> c0 < c2 fails -> 2
    #   5  0  0           1 2 2      (3,2): c0 = 0, c1 = 0, c2 = 5 -> c0 < c1 and c1 < c0 both fail -> 2, although c2 is the largest
    # back from (3,3): 2, 2, then column 1 upwards: the path enters the last row at key 0.
    x = np.asarray([[0, 5, 5],
                    [0, 0, 5],
                    [5, 0, 0]], np.float32)
    frames, path = ar.dtw(x)
    assert np.array_equal(frames, ar.dtw_fast(x))
    assert frames.tolist() == [0, 0, 0] and path == [(0, 0), (1, 0), (2, 0), (2, 1), (2, 2)]


def test_median_and_standardisation():
    z = np.asarray([[5.0, 1.0, 4.0, 2.0, 3.0, 9.0, 0.0, 7.0]])
    # reflect padding: [2 4 1 | 5 1 4 2 3 9 0 7 | 0 9 3]
    assert ar.median7_reflect(z).tolist() == [[2.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0]]
    assert ar.median7_reflect(z[:, :3]).tolist() == z[:, :3].tolist()          # three keys: unfiltered
    rng = np.random.default_rng(0)
    q = rng.standard_normal((5, 64)).astype(np.float16)
    k = rng.standard_normal((3, 64)).astype(np.float16)
    k[1] = 0
    k[1, 0] = -60.0
    q[:, 0] = 30.0                                                             # key 1 underflows to 0 in every row: std 0 -> Z 0, no NaN
    f = ar.head_weights(q, k)
    assert np.isfinite(f).all() and (f[:, 1] == 0).all()
    assert np.allclose(f[:, 0].mean(), 0, atol=1e-12) and np.allclose(f[:, 0].std(), 1, atol=1e-12)


def test_token_times():
    ids = [BEG + 10, 100, 101, SOLM, BEG + 200]
    assert ar.token_times(ids, [3, 40, 90], 1000, 1020, BEG, EOT) == [(1020, 1020), (1006, 1080), (1080, 1180), (1180, 1180), (1400, 1400)]


# ---------------------------------------------------------------------------------------------------------------------
# the host loop with a scripted aligner
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if not os.path.exists(os.path.join(HIP_DIR, "libwhisper_hip.so")):
        from whisper_amd import build
        build.build_hip()
    os.makedirs(BUILD, exist_ok=True)
    deps = SOURCES + HEADERS
    if not os.path.exists(DRIVER) or any(os.path.getmtime(d) > os.path.getmtime(DRIVER) for d in deps):
        cmd = ["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "whisper_amd", "host")] + SOURCES + \
              ["-o", DRIVER, "-L" + HIP_DIR, "-lwhisper_hip", "-Wl,-rpath," + HIP_DIR, "-lpthread"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout

    def run(flags, windows, max_len=0, mel_len=6000, with_pcm=0):
        args = [DRIVER, str(flags), str(max_len), str(mel_len), str(with_pcm)] + [",".join(map(str, ids)) + ";" + ",".join(map(str, fr)) for ids, fr in windows]
        r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout.strip().splitlines()[-1])
    return run


# window 1: two segments ([0.20 s] w100 w101 [4.00 s] / [4.00 s] w102 <solm> w103 w104 [10.00 s]); window 2 seeks to 10.00 s: one segment
W1 = ([BEG + 10, 100, 101, BEG + 200, BEG + 200, 102, SOLM, 103, 104, BEG + 500, EOT], [12, 60, 200, 230, 300, 410])
W2 = ([BEG, 105, 106, 107, BEG + 900, EOT], [0, 250, 600, 880])


def _expected(windows, seeks):
    out = []
    for (ids, frames), seek in zip(windows, seeks):
        kept = ids[:max(i for i, t in enumerate(ids) if t > BEG) + 1]          # the window keeps its tokens up to the last timestamp
        out.append((kept, frames, seek))
    return out


def test_times_from_frames_two_segments_and_two_windows(driver):
    got = driver(ALIGN_TOKENS | NO_CONTEXT, [W1, W2])
    assert got["hr"] == 0
    assert [c["seek"] for c in got["calls"]] == [0, 1000] and all(c["seekEnd"] == 6000 for c in got["calls"])          # once per window
    assert got["calls"][0]["sot"] == [SOT, EN, TRANSCRIBE] and got["calls"][0]["text"] == [100, 101, 102, 103, 104]
    assert got["calls"][1]["text"] == [105, 106, 107]
    segs = got["segments"]
    assert [(s["t0"], s["t1"]) for s in segs] == [(20, 400), (400, 1000), (1000, 2800)]                                 # segment times: the timestamps', unchanged
    assert [[t["id"] for t in s["tokens"]] for s in segs] == [[100, 101, BEG + 200], [102, SOLM, 103, 104, BEG + 500], [BEG, 105, 106, 107, BEG + 900]]          # a segment ends with its closing timestamp
    # window 1: the frames run on across its two segments
    f = W1[1]
    want = [ar.token_times([t["id"] for t in segs[0]["tokens"]], f[0:3], 0, segs[0]["t0"], BEG, EOT),
            ar.token_times([t["id"] for t in segs[1]["tokens"]], f[2:6], 0, segs[1]["t0"], BEG, EOT),
            ar.token_times([t["id"] for t in segs[2]["tokens"]], W2[1], 1000, segs[2]["t0"], BEG, EOT)]
    for s, w in zip(segs, want):
        assert [(t["t0"], t["t1"]) for t in s["tokens"]] == w
    assert want[1][1] == (2 * 230, 2 * 230)                                      # <solm>: the end of the text token before it
    assert want[0][0] == (24, 120) and want[0][2] == (400, 400)                   # a text token from its frames, a timestamp token its own time
    assert want[2][0] == (1000, 1000) and want[2][1] == (1000, 1500)              # window 2: seek 1000 + 2 x frame
    for s in segs:
        for t in s["tokens"]:
            assert t["t0"] <= t["t1"]
    # vlen: what TokenTimestamps puts there (" w100": a space and four characters, one of them... digits count 3)
    assert abs(segs[0]["tokens"][0]["vlen"] - (0.01 + 1.0 + 3 * 3.0)) < 1e-6


def test_a_special_token_first_in_its_segment_takes_the_segments_start(driver):
    got = driver(ALIGN_TOKENS | NO_CONTEXT, [([BEG + 50, SOLM, 100, BEG + 300, EOT], [70, 140])], mel_len=3000)
    seg = got["segments"][0]
    assert seg["t0"] == 100 and [t["id"] for t in seg["tokens"]] == [SOLM, 100, BEG + 300]
    assert [(t["t0"], t["t1"]) for t in seg["tokens"]] == [(100, 100), (140, 280), (600, 600)]


def test_a_range_that_is_not_emitted_does_not_shift_the_frames(driver):
    """Token 99 prints nothing, so [0.20 s] 99 [2.00 s] gives no segment; the next segment's text tokens are the window's second and third and take
    THEIR frames, not the first token's."""
    got = driver(ALIGN_TOKENS | NO_CONTEXT, [([BEG + 10, 99, BEG + 100, BEG + 100, 100, 101, BEG + 300, EOT], [5, 50, 80, 120])], mel_len=3000)
    assert got["calls"][0]["text"] == [99, 100, 101] and len(got["segments"]) == 1
    seg = got["segments"][0]
    assert [t["id"] for t in seg["tokens"]] == [100, 101, BEG + 300]
    assert [(t["t0"], t["t1"]) for t in seg["tokens"]] == [(100, 160), (160, 240), (600, 600)]


def test_aligner_is_never_called_without_the_flag(driver):
    got = driver(NO_CONTEXT, [W1, W2])
    assert got["hr"] == 0 and got["calls"] == []
    assert all(t["t0"] == -1 and t["t1"] == -1 for s in got["segments"] for t in s["tokens"])
    assert len(got["segments"]) == 3 and got["new_segments"] == 3


def test_max_len_wraps_on_the_aligned_times(driver):
    got = driver(ALIGN_TOKENS | NO_CONTEXT, [W1], max_len=10, mel_len=1000)
    # segment 2 of the window, " w102 w103 w104" (5 characters a word), max_len 10: " w102 w103" | " w104"; the cut is at w104's aligned t0
    segs = got["segments"]
    assert [s["text"] for s in segs] == [" w100 w101", " w102 w103", " w104"]
    assert (segs[1]["t0"], segs[1]["t1"]) == (400, 2 * 300) and (segs[2]["t0"], segs[2]["t1"]) == (2 * 300, 1000)
    assert got["new_segments"] == 3 and len(got["calls"]) == 1


def test_with_both_flags_the_aligned_times_win(driver):
    both = driver(ALIGN_TOKENS | TOKEN_TIMESTAMPS | NO_CONTEXT, [W1], mel_len=1000, with_pcm=1)
    only = driver(ALIGN_TOKENS | NO_CONTEXT, [W1], mel_len=1000)
    heur = driver(TOKEN_TIMESTAMPS | NO_CONTEXT, [W1], mel_len=1000, with_pcm=1)
    times = lambda g: [[(t["t0"], t["t1"]) for t in s["tokens"]] for s in g["segments"]]
    assert times(both) == times(only) != times(heur)
    assert [[t["vlen"] for t in s["tokens"]] for s in both["segments"]] == [[t["vlen"] for t in s["tokens"]] for s in heur["segments"]]
    assert [[t["vlen"] for t in s["tokens"]] for s in only["segments"]] == [[t["vlen"] for t in s["tokens"]] for s in heur["segments"]]
