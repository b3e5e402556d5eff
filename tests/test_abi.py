"""CPU tests of the drop-in boundary: the C-ABI library loads and exports every symbol include/whisper_hip.h declares.
No compute is called here (there is no GPU in the build container)."""
import ctypes
import os
import re

import pytest

from whisper_amd import binding, ggml_format as gf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    return sorted(set(re.findall(r"WH_API\s+[\w\s\*]+?\b(wh_\w+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    if not os.path.exists(binding.LIB_PATH):
        from whisper_amd import build
        build.build_hip()
    lib = ctypes.CDLL(binding.LIB_PATH)
    names = declared_symbols()
    assert len(names) >= 25
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert sorted(binding.EXPORTS) == names


def test_arena_layout_is_pure_function_of_hparams():
    """Ranks that only receive the RCCL broadcast rely on this: same hparams -> same byte count (no GPU needed)."""
    hp = gf.hparams_for("medium")
    n1 = binding.arena_bytes(hp)
    n2 = binding.arena_bytes(gf.hparams_for("medium"))
    assert n1 == n2
    # FP16 matrices dominate: ~ the size of the real ggml-medium.bin (1.53 GB) minus FP32 leftovers
    assert 1.4e9 < n1 < 1.7e9
    assert binding.arena_bytes(gf.hparams_for("large-v2")) > 2.9e9


def test_invalid_hparams_are_rejected():
    hp = gf.hparams_for("tiny")
    hp.n_audio_head = 5                     # 384 / 5 != 64
    with pytest.raises(binding.WhisperHipError):
        binding.arena_bytes(hp)


def test_no_silent_cpu_fallback():
    """Without a GPU, creating a model must fail loudly (WH_E_NO_DEVICE), never compute on the host."""
    if binding.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(binding.WhisperHipError):
        binding.HipModel(gf.hparams_for("test-d128"))


def test_product_never_touches_the_oracle():
    """oracle/ is the checker: nothing under whisper_amd/ (Python, C++ host, HIP) may import, include, link or execute it, and
    the bench uses it only in the cpu_baseline leg."""
    import re
    pkg = os.path.join(ROOT, "whisper_amd")
    offenders = []
    for base, _, files in os.walk(pkg):
        if os.sep + "lib" in base or "__pycache__" in base:
            continue
        for f in files:
            if not f.endswith((".py", ".cpp", ".h", ".hip")):
                continue
            text = open(os.path.join(base, f), errors="ignore").read()
            if f == "build.py":
                # the build script may BUILD the checker (make -C oracle); it must not import it
                text = re.sub(r'os\.path\.join\(ROOT, "oracle"\)|"oracle"', "", text)
            for m in re.finditer(r"^\s*(from|import)\s+oracle\b|#include\s+[\"<][^\">]*oracle|dlopen\([^)]*oracle|CDLL\([^)]*oracle", text, re.M):
                offenders.append((f, m.group(0)))
    assert not offenders, offenders
    bench = open(os.path.join(ROOT, "bench.py")).read()
    uses = [m.start() for m in re.finditer(r"from oracle import|import oracle", bench)]
    assert uses, "bench.py times the reference CPU path in its cpu_baseline leg"
    for u in uses:
        # every import sits inside cpu_baseline_worker / cpu_baseline
        head = bench[:u]
        assert head.rfind("def cpu_baseline") > head.rfind("def main") and head.rfind("def cpu_baseline") > head.rfind("def run_passes")


def test_decode_step_entry_points_reject_bad_arguments_before_any_launch():
    """wh_op_gemv_small / wh_op_cross_split / wh_op_self_block_dec: a null operand, or a shape their launchers do not take, is an error with a message and
    nothing is launched -- checked on the host alone (the pointers below are never dereferenced: every call is turned away first)."""
    import ctypes as C
    L = binding.lib()
    p = C.c_void_p(0x1000)
    one = C.c_float(1.0)

    def rejected(rc, word):
        msg = L.wh_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)

    # gemvSmall: no weight; an unknown prologue / epilogue; an operand its combination needs; shapes of the launcher
    rejected(L.wh_op_gemv_small(None, 1, 64, 64, 0, 0, None, p, None, None, None, None, None, None, p, None, None, None, None, 0, 0, 0, None, one), "gemv_small")
    rejected(L.wh_op_gemv_small(None, 1, 64, 64, 0, 2, p, p, None, None, None, None, None, None, p, None, None, None, None, 0, 0, 0, None, one), "gemv_small")
    rejected(L.wh_op_gemv_small(None, 1, 64, 64, 5, 0, p, p, None, None, None, None, None, None, p, None, None, None, None, 0, 0, 0, None, one), "gemv_small")
    rejected(L.wh_op_gemv_small(None, 1, 64, 64, 0, 1, p, None, p, p, None, None, None, None, p, None, None, None, None, 0, 0, 0, None, one), "gemv_small")
    rejected(L.wh_op_gemv_small(None, 1, 64, 64, 1, 0, p, p, None, None, None, None, None, None, None, p, None, None, None, 0, 0, 0, None, one), "GELU")
    rejected(L.wh_op_gemv_small(None, 1, 192, 64, 2, 1, p, None, p, p, p, None, p, None, None, None, p, p, p, 1, 448, 448, None, one), "nPast")
    rejected(L.wh_op_gemv_small(None, 5, 64, 64, 0, 0, p, p, None, None, None, None, None, None, p, None, None, None, None, 0, 0, 0, None, one), "gemvSmall")
    rejected(L.wh_op_gemv_small(None, 1, 64, 12, 0, 0, p, p, None, None, None, None, None, None, p, None, None, None, None, 0, 0, 0, None, one), "gemvSmall")
    rejected(L.wh_op_gemv_small(None, 1, 64, 8256, 0, 0, p, p, None, None, None, None, None, None, p, None, None, None, None, 0, 0, 0, None, one), "gemvSmall")
    rejected(L.wh_op_gemv_small(None, 1, 64, 4096, 0, 1, p, None, p, p, p, None, None, None, p, None, None, None, None, 0, 0, 0, None, one), "gemvSmall")
    rejected(L.wh_op_gemv_small(None, 1, 64, 72, 0, 3, p, None, None, None, None, p, None, None, p, None, None, None, None, 0, 0, 0, None, one), "gemvSmall")
    # the split cross-attention: a null scratch buffer; five sequences; more keys than rows; too many keys; too wide
    rejected(L.wh_op_cross_split(None, p, p, p, p, p, one, p, p, p, None, p, 1, 6, 1500, 1500), "cross_split")
    rejected(L.wh_op_cross_split(None, p, p, p, p, p, one, p, p, p, p, p, 5, 6, 1500, 1500), "crossSplit")
    rejected(L.wh_op_cross_split(None, p, p, p, p, p, one, p, p, p, p, p, 1, 6, 1500, 1499), "crossSplit")
    rejected(L.wh_op_cross_split(None, p, p, p, p, p, one, p, p, p, p, p, 1, 6, 1537, 1600), "crossSplit")
    rejected(L.wh_op_cross_split(None, p, p, p, p, p, one, p, p, p, p, p, 1, 21, 1500, 1500), "crossSplit")
    # selfBlockDec: a null cache; a position outside the cache; a cache deeper than its LDS score rows; too wide
    rejected(L.wh_op_self_block_dec(None, p, p, p, p, p, one, None, p, p, 1, 2, 448, 0, None), "self_block_dec")
    rejected(L.wh_op_self_block_dec(None, p, p, p, p, p, one, p, p, p, 1, 2, 448, 448, None), "self_block_dec")
    rejected(L.wh_op_self_block_dec(None, p, p, p, p, p, one, p, p, p, 1, 2, 448, -1, None), "self_block_dec")
    rejected(L.wh_op_self_block_dec(None, p, p, p, p, p, one, p, p, p, 1, 2, 513, 0, None), "selfBlockDec")
    rejected(L.wh_op_self_block_dec(None, p, p, p, p, p, one, p, p, p, 1, 21, 448, 0, None), "selfBlockDec")
    rejected(L.wh_op_self_block_dec(None, p, p, p, p, p, one, p, p, p, 0, 2, 448, 0, None), "selfBlockDec")


def test_encoder_product_entry_points_reject_bad_arguments_before_any_launch():
    """wh_op_gemm_encoder / wh_op_mel_to_conv_input: what the launchers cannot see -- a null operand of the epilogue, N against H, windows that are not whole, a V padding
    or a cache too small for what the product writes, overlapping output segments -- is an error with a message, checked on the host alone (the pointers below are
    never dereferenced: every call is turned away first)."""
    import ctypes as C
    import numpy as np
    B = binding
    p = 0x1000

    def rejected(word, **kw):
        args = dict(a=p, w=p, bias=p, M=256, N=384, K=128, lda=128, Mb=256, ldc=384, scale=1.0)
        args.update(kw)
        with pytest.raises(B.WhisperHipError, match=word):
            B.op_gemm_encoder(**args)

    rejected("Q/K/V needs", epi=B.EPI_QKV_ENC, q=p, k=p, T=128, Tpad=256, H=2)
    rejected("3 \\* 64 \\* H", epi=B.EPI_QKV_ENC, q=p, k=p, v=p, T=128, Tpad=256, H=3)
    rejected("M % T", epi=B.EPI_QKV_ENC, q=p, k=p, v=p, T=100, Tpad=256, H=2)
    rejected("Tpad", epi=B.EPI_QKV_ENC, q=p, k=p, v=p, T=128, Tpad=127, H=2)
    rejected("Tpad", epi=B.EPI_QKV_ENC, q=p, k=p, v=p, T=128, Tpad=136, H=2)
    rejected("cross-K/V needs", epi=B.EPI_CROSS_KV, k=p, T=128, H=2, B=2)
    rejected("2 \\* 64 \\* H", epi=B.EPI_CROSS_KV, k=p, v=p, T=128, H=2, B=2)
    rejected("B must hold", epi=B.EPI_CROSS_KV, k=p, v=p, N=512, T=128, H=2, B=1)
    rejected("conv2 needs", epi=B.EPI_CONV2, out32=p)
    rejected("whole segments", epi=B.EPI_F16_GELU, out16=p, Mb=100)
    rejected("do not overlap", epi=B.EPI_F16_GELU, out16=p, Mb=128, cBatchStride=127 * 384)
    rejected("ldc >= N", epi=B.EPI_F16_GELU, out16=p, ldc=383)
    rejected("must not be null", epi=B.EPI_F16_GELU)
    rejected("unknown epilogue", epi=5)
    rejected("K a positive multiple of 64", epi=B.EPI_F16_GELU, out16=p, K=96)
    rejected("16-byte aligned", epi=B.EPI_F16_GELU, out16=p, lda=100)
    L = B.lib()
    for args in ((None, p, 0, 100, None, None, None, 1000, 80, 10, 1),            # no output
                 (None, p, 0, 100, None, None, p, 959, 80, 10, 1),                # the window does not fit its stride
                 (None, None, 0, 100, None, None, p, 960, 80, 10, 1),             # no spectrogram
                 (None, p, 0, 0, None, None, p, 960, 80, 10, 1)):                 # no length
        assert L.wh_op_mel_to_conv_input(*args) != 0 and b"mel_to_conv_input" in L.wh_last_error()
    neg = np.array([-1], np.int32)
    assert L.wh_op_mel_to_conv_input(None, p, 0, 100, neg.ctypes.data, None, p, 960, 80, 10, 1) != 0 and b"negative" in L.wh_last_error()
    wins = (B.MelWindowC * 1)(B.MelWindowC(p, 100, -1, 0))
    assert L.wh_op_mel_to_conv_input(None, None, 0, 0, None, C.cast(wins, C.c_void_p), p, 960, 80, 10, 1) != 0 and b"bad window" in L.wh_last_error()


def test_tuning_bits_of_the_binding_match_the_library_header():
    """whisper_amd/binding.py mirrors csrc/kernels.h eTuning by hand; tests restore binding.TUNE_DEFAULT after an A/B, so a bit that is in one default
    and not in the other would silently change what the rest of a test session measures."""
    import re
    from whisper_amd import binding
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "whisper_amd", "csrc", "kernels.h")).read()
    body = text[text.index("enum eTuning"):]
    body = body[:body.index("};")]
    values = {}
    for name, expr in re.findall(r"^\s*(TUNE_[A-Z0-9_]+)\s*=\s*([^,/\n]+?)\s*,?\s*(?://.*)?$", body, re.M):
        expr = re.sub(r"(\d+)u\b", r"\1", expr)
        values[name] = eval(expr, {}, values)
    assert "TUNE_DEFAULT" in values and len(values) > 25
    for name, v in values.items():
        assert hasattr(binding, name), name + " is missing in binding.py"
        assert getattr(binding, name) == v, (name, getattr(binding, name), v)


def test_option_defaults_of_the_binding_match_the_library():
    """binding.OPTION_DEFAULTS mirrors the initialisers of csrc/kernels.h `struct Options` by hand, and tests restore an option from it after an A/B: a value that differs
    from the library's compiled-in default would silently change what the rest of a session runs. Read back from the library itself (wh_debug_get_option is host code) in
    a child process without WH_OPT_* variables, so that neither this session's environment nor an earlier test's set_option is in the way."""
    import subprocess
    import sys
    code = ("import json; from whisper_amd import binding; "
            "print(json.dumps({k: binding.get_option(k) for k in binding.OPTION_DEFAULTS}))")
    env = {k: v for k, v in os.environ.items() if not k.startswith("WH_OPT_")}
    env["PYTHONPATH"] = ROOT
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    import json
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got == binding.OPTION_DEFAULTS, {k: (got[k], v) for k, v in binding.OPTION_DEFAULTS.items() if got[k] != v}
    # every option the library knows is mirrored (the names are listed in the header's comment of wh_debug_set_option)
    text = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    at = text.index("WH_API int wh_debug_set_option")
    listed = set(re.findall(r'"([a-z0-9_]+)"', text[at - 2000:at]))
    assert set(binding.OPTION_DEFAULTS) <= listed | {"enc_ablate"}, sorted(set(binding.OPTION_DEFAULTS) - listed)
    with pytest.raises(RuntimeError):
        binding.get_option("no_such_option")
