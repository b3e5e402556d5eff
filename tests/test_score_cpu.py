"""CPU tests of scoring a given transcript ("Scoring"): the float64 restatement pinned by hand-made rows, the fixture of the GPU tests held
against the generator's constants, and the declarations. The GPU twin: tests/test_gpu_score.py."""
import ctypes as C
import json
import math
import os
import re

import numpy as np

import token_score_ref as TS
from whisper_amd import binding

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NINF = -np.inf


def test_the_restatement_on_hand_made_rows():
    """ties at the maximum; a tie between the target and a lower id; target = arg-max; -inf entries; a target at -inf"""
    ln = math.log
    # four equal entries: every id has probability 1/4; the arg-max is id 0 and the rank of id k is k
    for t in range(4):
        lp, blp, best, rank = TS.score_row([2.0, 2.0, 2.0, 2.0], t)
        assert abs(lp + ln(4)) < 1e-15 and abs(blp + ln(4)) < 1e-15 and best == 0 and rank == t
    # ties at the maximum (ids 1 and 3): best is the lower id; the target at the higher one has rank 1 and the arg-max's log-probability
    x = [0.0, 5.0, NINF, 5.0, 1.0]
    s = 2.0 + math.exp(-5.0) + math.exp(-4.0)
    assert TS.score_row(x, 1) == (-ln(s), -ln(s), 1, 0)
    assert TS.score_row(x, 3) == (-ln(s), -ln(s), 1, 1)
    lp, blp, best, rank = TS.score_row(x, 4)
    assert abs(lp - (-4.0 - ln(s))) < 1e-15 and blp == -ln(s) and best == 1 and rank == 2
    # a target at -inf scores -inf with a finite bestLogprob; the -inf entry adds nothing to the sum; every finite id outranks it
    lp, blp, best, rank = TS.score_row(x, 2)
    assert lp == NINF and blp == -ln(s) and best == 1 and rank == 4
    # two -inf entries tie among themselves: the lower id first
    assert TS.score_row([NINF, 1.0, NINF], 2)[3] == 2 and TS.score_row([NINF, 1.0, NINF], 0)[3] == 1
    # a tie between the target and a lower id that is not the maximum
    x = [3.0, 1.5, 7.0, 1.5, 1.5]
    assert [TS.score_row(x, t)[3] for t in range(5)] == [1, 2, 0, 3, 4] and TS.score_row(x, 3)[2] == 2
    # target = arg-max: logprob == bestLogprob, rank 0; a row far from zero does not overflow
    lp, blp, best, rank = TS.score_row(np.array([1000.0, 1001.0, 999.0], np.float32), 1)
    want = -ln(1.0 + math.exp(-1.0) + math.exp(-2.0))
    assert lp == blp and abs(lp - want) < 1e-15 and best == 1 and rank == 0
    # the probabilities of a row sum to one
    rng = np.random.default_rng(3)
    x = (4.0 * rng.standard_normal(500)).astype(np.float32)
    x[::7] = NINF
    got = TS.score_rows(np.tile(x, (500, 1)), np.arange(500))
    assert abs(np.exp(got["logprob"]).sum() - 1.0) < 1e-12 and sorted(got["rank"]) == list(range(500))
    assert (got["best"] == int(np.argmax(x))).all() and np.allclose(got["bestLogprob"], got["logprob"].max())


def test_the_fixture_is_the_generators():
    """tests/golden/ref_score_d128.json against tests/golden/make_golden_score.py: seeds, lengths and first scored entries; the restatement of the reference's
    numerics itself stays inside the 2 % cap on order exceptions, which is what the seeds were chosen for."""
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden_score as mk
    with open(os.path.join(HERE, "golden", "ref_score_d128.json")) as f:
        g = json.load(f)
    assert (g["model_seed"], g["mel_seed"]) == (mk.MODEL_SEED, mk.MEL_SEED)
    assert tuple(len(w["row"]) for w in g["windows"]) == mk.LENS == (5, 12, 40) and tuple(w["first"] for w in g["windows"]) == mk.FIRST
    n = sum(len(w["entries"]) for w in g["windows"])
    assert n == sum(a - b for a, b in zip(mk.LENS, mk.FIRST)) and n > 32            # the product crosses the 32-row boundary
    assert g["np_rank_or_best_differs"] <= 0.02 * n
    w = g["windows"][2]
    assert w["bad"] == mk.corrupted(w["row"], w["first"]) and sum(a != b for a, b in zip(w["bad"], w["row"])) >= (len(w["entries"]) - 2) // 3
    d = [abs(e["np_logprob"] - e["logprob"]) for x in g["windows"] for e in x["entries"]]
    assert max(d) == g["np_logprob_dist_max"] and abs(np.mean(d) - g["np_logprob_dist_mean"]) < 1e-15


def test_declarations():
    """The record is 16 bytes on both sides of the ABI, the entry points are exported, the options are registered with the defaults of kernels.h and named on the
    option list of wh_debug_set_option's comment; the logits buffer of the feature stays under 64 MiB at the largest vocabulary."""
    assert C.sizeof(binding.TokenScoreC) == 16 == binding.TOKEN_SCORE_DTYPE.itemsize
    assert [f[0] for f in binding.TokenScoreC._fields_] == list(binding.TOKEN_SCORE_DTYPE.names) == ["logprob", "bestLogprob", "best", "rank"]
    assert "wh_score_tokens" in binding.EXPORTS and "wh_op_token_scores" in binding.EXPORTS
    L = binding.lib()
    assert L.wh_score_tokens and L.wh_op_token_scores
    assert binding.get_option("score_chunk_rows") == binding.OPTION_DEFAULTS["score_chunk_rows"] == 320 and binding.get_option("score_regs") == 1
    assert 320 * 51866 * 4 < 64 << 20
    with open(os.path.join(ROOT, "include", "whisper_hip.h")) as f:
        header = f.read()
    listed = re.search(r"Integer knobs beyond the 32 switches(.*?)WH_API int wh_debug_set_option", header, re.S).group(1)
    assert '"score_chunk_rows"' in listed and '"score_regs"' in listed
    assert re.search(r"typedef struct wh_token_score\s*\{\s*float logprob, bestLogprob;\s*int32_t best, rank;\s*\} wh_token_score;", header)
    # argument checks that need no device: null pointers and empty shapes are refused before anything is touched
    assert L.wh_op_token_scores(None, None, 10, 1, 10, None, None) == -1
    assert L.wh_score_tokens(None, 1, None, None, None, 4, None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# scoreRequest.h through tests/score_cpu/driver.cpp, a program of its own under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------
def test_the_rules_of_a_request_as_a_program_of_its_own():
    """Row building, every refusal, packing 1 / 5 / 7 requests into 1 / 2 / 5 slots and back in request order (a failing request among them), the aligned
    times: host code only, with its own main, built with -fsanitize=address,undefined and run directly."""
    import shutil
    import subprocess
    import pytest
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    build = os.path.join(HERE, "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "score-driver")
    src = os.path.join(HERE, "score_cpu", "driver.cpp")
    hdrs = [os.path.join(ROOT, "whisper_amd", "host", "scoreRequest.h"), os.path.join(ROOT, "include", "whisperApi.h"), os.path.join(ROOT, "include", "whisper_hip.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in [src] + hdrs):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(ROOT, "whisper_amd", "host"), src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout, r.stderr[-2000:])
    assert int(r.stdout.split()[1]) > 500


def test_flat_c_argument_checks_and_exports():
    """The flat C entries exist and refuse null objects before anything is touched; the Python faces exist; the record is 32 bytes on both sides."""
    from whisper_amd import api
    E_POINTER = 0x80004003
    L = api.lib()
    n = C.c_uint32(0)
    assert L.whisperc_sot_sequence(None, b"en", 0, 0, None, 0, C.byref(n)) & 0xFFFFFFFF == E_POINTER
    assert L.whisperc_score_tokens(None, None, 0, None, 0, None, 0, 0, None) & 0xFFFFFFFF == E_POINTER
    assert L.whisperc_batch_score(None, 0, None, None, None, None, None, None, None, None, 0, None, None) & 0xFFFFFFFF == E_POINTER
    assert callable(api.Context.score) and callable(api.BatchRunner.score) and callable(api.Model.sot_sequence) and callable(binding.HipContext.score_tokens)
    assert api.TOKEN_SCORE_DT.itemsize == 32 and api.TOKEN_SCORE_DT.names[:4] == ("logprob", "best_logprob", "best", "rank")
    with open(os.path.join(ROOT, "include", "whisper_c.h")) as f:
        header = f.read()
    for name in ("whisperc_sot_sequence", "whisperc_score_tokens", "whisperc_batch_score"):
        assert re.search(r"int32_t %s\(" % name, header), name


def test_whisper_main_takes_the_option():
    """--score FILE is parsed out before the reference's parser sees the line: --dump-options and the usage text stay the reference's."""
    import subprocess
    from whisper_amd import build
    if not os.path.exists(build.CLI_BIN):
        build.build_all()
    run_main = lambda *a: subprocess.run([build.CLI_BIN] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    plain = run_main("--dump-options", "-f", "a.wav")
    with_it = run_main("--dump-options", "--score", "a.txt", "-f", "a.wav")
    assert plain.returncode == 0 and with_it.returncode == 0 and with_it.stdout == plain.stdout and "a.wav" in plain.stdout
    usage = run_main("-h")
    assert "--score" not in usage.stdout + usage.stderr
    missing = run_main("-f", "a.wav", "--score")
    assert missing.returncode == 2 and "--score needs a file" in missing.stderr
