"""CPU tests of the INT8 decoder weights' public face: the two entries are exported, wh_op_gemv_w8 turns bad calls away on the host, whisper-mgpu takes the option."""
import ctypes as C
import os
import subprocess

import pytest

from whisper_amd import binding


def test_entries_are_exported():
    L = C.CDLL(binding.LIB_PATH)
    for name in ("wh_context_set_decoder_w8", "wh_op_gemv_w8"):
        assert name in binding.EXPORTS and hasattr(L, name)


# ( M, K, pro, operands present ): null operands, K no multiple of 128, too many rows, too many rows for the LayerNorm prologue
@pytest.mark.parametrize("M,K,pro,present", [(1, 128, 0, False), (1, 100, 0, True), (129, 128, 0, True), (33, 128, 1, True)])
def test_gemv_w8_rejects_before_any_launch(M, K, pro, present):
    """Each returns -1 with a message naming the kernel; the pointers are never dereferenced."""
    p = C.c_void_p(0x1000) if present else None
    rc = binding.lib().wh_op_gemv_w8(None, M, 64, K, 0, pro, p, p, p, p, p, p, None, None, C.c_void_p(0x1000), None, None, None, None, 0, 0, 0, None, C.c_float(1.0))
    assert rc == -1 and "gemvW8" in binding.lib().wh_last_error().decode()


def test_mgpu_takes_the_option():
    """-decoder-int8 parses (the line then fails for its missing -m and -f, not with the usage text an unknown option gets)."""
    from whisper_amd import build
    if not os.path.exists(build.MGPU_BIN):
        build.build_all()
    for name in ("-decoder-int8", "--decoder-int8"):
        r = subprocess.run([build.MGPU_BIN, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 1 and "-m and -f are required" in r.stderr and "usage:" not in r.stderr
    r = subprocess.run([build.MGPU_BIN, "-decoder-int9"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 1 and "usage: whisper-mgpu" in r.stderr and "-decoder-int8" in r.stderr
