"""Constrained decoding on the host, no device needed: api.compile_phrases against a plain statement of its language and against host/phraseAutomaton.h, and
optionRules::checkConstraint through Whisper::setBatchDecodingConstraint on the scheduler over the test double of the compute layer."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import constraint_ref as R
import test_hostloop_cpu as H
from whisper_amd import api, ggml_format as gf

PHRASES = ["lights on", "lights off", "stop", "a", "a b", "café"]
LEADS = ["optional", "always", "never"]
E_INVALIDARG, E_NOTIMPL = 0x80070057, 0x80004001


def _splits(text):
    """text is phrases joined by single spaces"""
    return any(text == p or (text.startswith(p + " ") and _splits(text[len(p) + 1:])) for p in PHRASES)


@pytest.mark.parametrize("repeat", [False, True])
@pytest.mark.parametrize("lead", LEADS)
def test_compile_phrases_reads_its_language(lead, repeat):
    """Accepted: a phrase -- under repeat, phrases joined by single spaces -- behind one space, no space, or either, as leading_space says. Nothing else."""
    class_of, trans, accept, start = api.compile_phrases(PHRASES, lead, repeat)
    for text in ("stop", " stop", "  stop", "lights o", "lights on stop", "stop a b a", "a b", " a b", "a  b", "stopp", "stop ", " café", " ", ""):
        spaced = text.startswith(" ")
        body = text[1:] if spaced else text
        want = (lead == "optional" or (lead == "always") == spaced) and (_splits(body) if repeat else body in PHRASES)
        s = R.walk_bytes(class_of, trans, start, text.encode())
        assert (s >= 0 and bool(accept[s])) == want, text
        if want:                                                                 # ... and every prefix of an accepted text is read
            assert all(R.walk_bytes(class_of, trans, start, text.encode()[:i]) >= 0 for i in range(len(text.encode())))
    with pytest.raises(ValueError):
        api.compile_phrases([])
    with pytest.raises(ValueError):
        api.compile_phrases(["x"], "sometimes")


@pytest.fixture(scope="module")
def lib():
    """whisper_amd/host/batchScheduler.cpp compiled UNCHANGED next to the unchanged test double of the compute layer and tests/constraint_cpu/rules_driver.cpp"""
    ref = os.path.join(H.REF_DIR, "libwhisper_ref.so")
    if not os.path.exists(ref) or shutil.which("g++") is None:
        pytest.skip("oracle/_ref/libwhisper_ref.so not built, or no g++")
    host = os.path.join(H.ROOT, "whisper_amd", "host")
    out = os.path.join(H.BUILD, "libconstraint_cpu.so")
    srcs = [os.path.join(H.ROOT, "tests", "constraint_cpu", "rules_driver.cpp")] + [os.path.join(host, f) for f in ("batchScheduler.cpp", "support.cpp", "tokenTimestamps.cpp")]
    deps = srcs + [os.path.join(host, f) for f in os.listdir(host) if f.endswith(".h")] + [os.path.join(H.ROOT, "tests", "hostloop_cpu", f) for f in ("fake_device.cpp", "batch_driver.cpp")]
    os.makedirs(H.BUILD, exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps + [ref]):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + os.path.join(H.ROOT, "include"), "-I" + host] + srcs +
                           ["-o", out, "-L" + H.REF_DIR, "-lwhisper_ref", "-Wl,-rpath," + H.REF_DIR, "-Wl,-Bsymbolic", "-Wl,--no-undefined", "-lpthread"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.cc_rules.argtypes = [C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int, C.c_int32, C.c_int, C.c_float]
    L.cc_automaton.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.cc_result.restype = C.c_char_p
    return L


@pytest.mark.parametrize("repeat", [False, True])
@pytest.mark.parametrize("lead", LEADS)
def test_the_cpp_automaton_is_the_python_one(lib, lead, repeat):
    """host/phraseAutomaton.h, which whisper-main --allow-phrases runs, against api.compile_phrases: the same arrays, state for state."""
    lib.cc_automaton("\n".join(PHRASES).encode(), LEADS.index(lead), int(repeat))
    got = json.loads(lib.cc_result().decode())
    class_of, trans, accept, start = api.compile_phrases(PHRASES, lead, repeat)
    assert start == 0 and got["class_of"] == class_of.tolist() and got["trans"] == trans.tolist() and got["accept"] == accept.tolist()


def test_option_rules(lib, tmp_path):
    """optionRules::checkConstraint behind setBatchDecodingConstraint: the limits, a transition and a class out of range, the start, the penalty -- E_INVALIDARG;
    what lies inside them and nullptr -- S_OK; and, on a scheduler that was not given the device entry, E_NOTIMPL for a constraint and S_OK for nullptr."""
    path = str(tmp_path / "m.bin")
    gf.write_model(path, gf.conditioned_model(gf.conditioned_layout(gf.hparams_for("test-d128-ml")), 4, kind="test-d128-ml", seed=10))
    inf, nan = float("inf"), float("nan")

    def rules(hook=1, states=2, classes=3, start=0, fill=-1, at=-1, value=0, cls=0, penalty=100.0):
        return lib.cc_rules(path.encode(), hook, states, classes, start, fill, at, value, cls, penalty) & 0xFFFFFFFF

    good = [dict(), dict(penalty=inf), dict(states=4096, classes=16, fill=4095), dict(states=256, classes=256), dict(states=1, classes=1, fill=0), dict(states=0),
            dict(at=5, value=1), dict(cls=2), dict(start=1)]
    bad = [dict(states=4097, classes=1), dict(classes=257, states=1), dict(states=300, classes=256), dict(at=5, value=2), dict(at=0, value=-2), dict(cls=3), dict(start=2),
           dict(penalty=0.0), dict(penalty=-1.0), dict(penalty=nan)]
    assert [rules(**kw) for kw in good] == [0] * len(good)
    assert [rules(**kw) for kw in bad] == [E_INVALIDARG] * len(bad)
    assert rules(hook=0) == E_NOTIMPL and rules(hook=0, states=0) == 0 and rules(hook=0, penalty=nan) == E_INVALIDARG
