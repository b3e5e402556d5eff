"""CPU tests of the quantized ggml models: the block formats of whisper_amd/ggml_format.py (QTensor, dequantize, quantize, quantize_model, the file round
trip, dequantized_twin), python -m whisper_amd.quantize, and whisper_amd/host/ggmlTensor.h through tests/quant_cpu/driver.cpp, a program of its own under
the sanitizers.

The contract (include/whisper_hip.h: wh_dequantize): a quantized matrix is the FP16 matrix of fp16( (float)d * (float)( q - off ) ) resp.
fp16( (float)d * (float)q + (float)m ). The product is exact in FP32 (11 x 8 significant bits), so the independent evaluation here is float64 -- in which the
sum is exact too: d q and m are multiples of 2^-24 below 2^22 -- rounded to float32 and then to float16; no tolerance, bits are compared."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from whisper_amd import ggml_format as gf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
TYPES = ("q4_0", "q4_1", "q5_0", "q5_1", "q8_0")


def f16_bytes(v):
    return np.asarray([v], "<f2").tobytes()


def make_block(qtype, d, m, q):
    """One block from the table of the format: q holds the 32 quants as the type stores them (0 .. 15, 0 .. 31 or -128 .. 127)"""
    q = list(q)
    assert len(q) == 32
    if qtype == "q8_0":
        return f16_bytes(d) + struct.pack("<32b", *q)
    head = f16_bytes(d) + (f16_bytes(m) if qtype.endswith("_1") else b"")
    if qtype.startswith("q5"):
        head += struct.pack("<I", sum(((v >> 4) & 1) << i for i, v in enumerate(q)))
    return head + bytes((q[j] & 15) | ((q[j + 16] & 15) << 4) for j in range(16))


def test_hand_made_blocks():
    """Each type's block, written byte by byte from the format's table, gives the values the table states"""
    # the worked q5_0 block: d = 1.0 (0x3C00), qh = 01 00 01 00, qs[0] = 0x21, every other qs 0
    worked = bytes([0x00, 0x3C, 0x01, 0x00, 0x01, 0x00, 0x21] + [0] * 15)
    want = np.full(32, -16.0, np.float32)
    want[0], want[16] = 1.0, 2.0
    got = gf.dequantize(gf.QTensor("q5_0", (32,), np.frombuffer(worked, np.uint8)))
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert make_block("q5_0", 1.0, None, [17] + [0] * 15 + [18] + [0] * 15) == worked

    ramp4 = [(5 * i + 3) % 16 for i in range(32)]
    ramp5 = [(7 * i + 5) % 32 for i in range(32)]
    ramp8 = [-128, 127] + [(37 * i) % 256 - 128 for i in range(30)]
    cases = {
        "q4_0": (0.5, None, ramp4, [0.5 * (v - 8) for v in ramp4], 18),
        "q4_1": (0.25, -3.0, ramp4, [0.25 * v - 3.0 for v in ramp4], 20),
        "q5_0": (-2.0, None, ramp5, [-2.0 * (v - 16) for v in ramp5], 22),
        "q5_1": (0.125, 10.0, ramp5, [0.125 * v + 10.0 for v in ramp5], 24),
        "q8_0": (0.0625, None, ramp8, [0.0625 * v for v in ramp8], 34),
    }
    for qtype, (d, m, q, values, size) in cases.items():
        raw = make_block(qtype, d, m, q)
        assert len(raw) == size == gf.BLOCK_BYTES[qtype]
        # two blocks, the second with the quants reversed: element order inside and across blocks
        raw2 = raw + make_block(qtype, d, m, q[::-1])
        qt = gf.QTensor(qtype, (2, 32), np.frombuffer(raw2, np.uint8))
        want = np.asarray([values, values[::-1]], np.float32)
        assert np.array_equal(gf.dequantize(qt), want), qtype
        assert np.array_equal(gf.dequantize_f16(qt), want.astype(np.float16)) and gf.dequantize_f16(qt).dtype == np.float16
    with pytest.raises(ValueError):
        gf.QTensor("q4_0", (48,), np.zeros(27, np.uint8))
    with pytest.raises(ValueError):
        gf.QTensor("q4_0", (32,), np.zeros(17, np.uint8))
    with pytest.raises(ValueError):
        gf.QTensor("q4_2", (32,), np.zeros(18, np.uint8))


def independent_f16(qtype, raw):
    """The values of the blocks, parsed byte by byte and evaluated in float64 (exact), rounded to float32 and then to float16"""
    size = gf.BLOCK_BYTES[qtype]
    out = []
    for o in range(0, len(raw), size):
        b = raw[o:o + size]
        d = float(np.frombuffer(b[0:2], "<f2")[0])
        pos = 2
        m = None                                             # no term at all for the _0 types: -0.0 + 0.0 would lose the sign of a zero
        if qtype.endswith("_1"):
            m = float(np.frombuffer(b[2:4], "<f2")[0])
            pos = 4
        if qtype == "q8_0":
            q = [v - 256 if v > 127 else v for v in b[2:34]]
        else:
            qh = 0
            if qtype.startswith("q5"):
                qh = int.from_bytes(b[pos:pos + 4], "little")
                pos += 4
            qs = b[pos:pos + 16]
            q = [(qs[j] & 15) | (((qh >> j) & 1) << 4) for j in range(16)] + [(qs[j] >> 4) | (((qh >> (j + 16)) & 1) << 4) for j in range(16)]
        off = {"q4_0": 8, "q5_0": 16}.get(qtype, 0)
        out += [d * (v - off) if m is None else d * v + m for v in q]
    with np.errstate(over="ignore"):
        return np.asarray(out, np.float64).astype(np.float32).astype(np.float16)


@pytest.mark.parametrize("qtype", TYPES)
def test_random_blocks_against_float64(qtype):
    """Random bytes with random finite FP16 d and m -- every exponent, subnormals included, both signs -- : the same bits as the float64 evaluation"""
    rng = np.random.default_rng(11 + gf.GGML_TYPES[qtype])
    n, size = 600, gf.BLOCK_BYTES[qtype]
    raw = rng.integers(0, 256, (n, size), dtype=np.uint8)

    def finite_half(count):
        bits = rng.integers(0, 1 << 16, count).astype(np.uint16)
        bits[(bits & 0x7C00) == 0x7C00] &= 0xBFFF            # inf and NaN become finite
        bits[:count // 6] &= 0x83FF                          # a sixth of them subnormal (or zero)
        return bits

    raw[:, 0:2] = finite_half(n).astype("<u2").view(np.uint8).reshape(n, 2)
    if qtype.endswith("_1"):
        raw[:, 2:4] = rng.permutation(finite_half(n)).astype("<u2").view(np.uint8).reshape(n, 2)
    d16 = raw[:, 0:2].copy().view("<f2").reshape(-1)
    assert np.isfinite(d16).all() and ((d16 != 0) & (np.abs(d16) < 6.2e-5)).sum() > 50
    qt = gf.QTensor(qtype, (n, 32), raw)
    got = gf.dequantize_f16(qt)
    want = independent_f16(qtype, raw.tobytes()).reshape(n, 32)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    # subnormal results and overflow both occur and are kept
    assert ((got != 0) & (np.abs(got) < 6.2e-5)).any() and np.isinf(got).any()
    # the float32 stage is exact for the _0 types
    if not qtype.endswith("_1"):
        assert np.array_equal(gf.dequantize(qt).astype(np.float64), (d16.astype(np.float64)[:, None] * (gf._block_fields(qt)[2] - {"q4_0": 8, "q5_0": 16}.get(qtype, 0))))


@pytest.mark.parametrize("qtype", TYPES)
def test_quantize_follows_the_reference_rows(qtype):
    """The scale and a few quants of a block computed by hand, the error bound of the grid, and ggml's corner cases: an all-zero block, ties of the maximum"""
    rng = np.random.default_rng(5)
    x = (0.05 * rng.standard_normal((40, 64))).astype(np.float32)
    x[3, :32] = 0
    qt = gf.quantize(x, qtype)
    assert qt.shape == (40, 64) and qt.blocks.size == 80 * gf.BLOCK_BYTES[qtype]
    y = gf.dequantize(qt)
    blocks = x.reshape(-1, 32)
    d16 = qt.blocks.reshape(80, -1)[:, 0:2].copy().view("<f2").reshape(-1).astype(np.float32)
    if qtype in ("q4_0", "q5_0"):
        k = 8 if qtype == "q4_0" else 16
        big = blocks[np.arange(80), np.abs(blocks).argmax(axis=1)]
        assert np.array_equal(d16, (big / np.float32(-k)).astype(np.float16).astype(np.float32))
    elif qtype == "q8_0":
        assert np.array_equal(d16, (np.abs(blocks).max(axis=1) / np.float32(127)).astype(np.float16).astype(np.float32))
    else:
        k = 15 if qtype == "q4_1" else 31
        assert np.array_equal(d16, ((blocks.max(axis=1) - blocks.min(axis=1)) / np.float32(k)).astype(np.float16).astype(np.float32))
    # one step of the grid (half a step for the rounding, the rest for d and m stored as FP16)
    step = np.abs(d16)[:, None]
    assert (np.abs(y.reshape(-1, 32) - blocks) <= step * 1.01 + 1e-3 * np.abs(blocks).max(axis=1, keepdims=True)).all()
    assert np.array_equal(y[3, :32], np.zeros(32, np.float32))
    with pytest.raises(ValueError):
        gf.quantize(np.zeros((4, 48), np.float32), qtype)


@pytest.mark.parametrize("qtype", ["q8_0", "q4_0"])
def test_quantize_of_dequantized_values_is_idempotent(qtype):
    rng = np.random.default_rng(8)
    x = rng.standard_normal((64, 128)).astype(np.float32) * np.float32(0.07)
    q1 = gf.quantize(x, qtype)
    q2 = gf.quantize(gf.dequantize(q1), qtype)
    assert np.array_equal(q1.blocks, q2.blocks)
    assert np.array_equal(gf.dequantize(q1), gf.dequantize(q2))


@pytest.fixture(scope="module")
def small_model():
    return gf.synth_model("test-d128", seed=21)


@pytest.mark.parametrize("qtype", TYPES)
def test_quantize_model_selects_the_matrices(small_model, qtype):
    """Exactly the 2-D *.weight matrices are quantized: conv weights, positional embeddings, biases and LayerNorm vectors are the same objects as before"""
    qm = gf.quantize_model(small_model, qtype)
    assert qm.hparams.f16 == 2000 + gf.GGML_FTYPES[qtype] and small_model.hparams.f16 == 1
    assert gf.split_ftype(qm.hparams.f16) == (2, gf.GGML_FTYPES[qtype])
    n_q = 0
    for name, shape, is_f16 in gf.tensor_specs(small_model.hparams):
        a = qm.tensors[name]
        linear = name.endswith(".weight") and len(shape) == 2
        if linear:
            assert isinstance(a, gf.QTensor) and a.qtype == qtype and a.shape == tuple(shape), name
            n_q += 1
        else:
            assert a is small_model.tensors[name], name
    for name in ("encoder.conv1.weight", "encoder.conv2.weight", "encoder.positional_embedding", "decoder.positional_embedding", "encoder.conv1.bias",
                 "decoder.ln.weight", "encoder.ln_post.weight", "encoder.blocks.0.attn_ln.weight", "decoder.blocks.1.mlp.0.bias"):
        assert not isinstance(qm.tensors[name], gf.QTensor), name
    hp = small_model.hparams
    assert n_q == 1 + 6 * hp.n_audio_layer + 10 * hp.n_text_layer and isinstance(qm.tensors["decoder.token_embedding.weight"], gf.QTensor)
    with pytest.raises(ValueError):
        gf.quantize_model(qm, qtype)
    twin = gf.dequantized_twin(qm)
    assert twin.hparams.f16 == 1
    for name, a in twin.tensors.items():
        assert isinstance(a, np.ndarray) and a.dtype == small_model.tensors[name].dtype and a.shape == small_model.tensors[name].shape
        if isinstance(qm.tensors[name], gf.QTensor):
            assert np.array_equal(a.view(np.uint16), gf.dequantize_f16(qm.tensors[name]).view(np.uint16))


@pytest.mark.parametrize("qtype", TYPES)
def test_quantized_file_round_trip(small_model, tmp_path, qtype):
    """write_model, read_model, write_model: the same bytes; the size is the header plus the sum of the record sizes"""
    qm = gf.quantize_model(small_model, qtype)
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    size = gf.write_model(a, qm)
    back = gf.read_model(a)
    assert back.hparams == qm.hparams and list(back.tensors) == [n for n, _, _ in gf.tensor_specs(qm.hparams)]
    for name, t in qm.tensors.items():
        r = back.tensors[name]
        if isinstance(t, gf.QTensor):
            assert isinstance(r, gf.QTensor) and r.qtype == qtype and r.shape == t.shape and np.array_equal(r.blocks, t.blocks)
        else:
            assert np.array_equal(r, t) and r.dtype == t.dtype
    assert gf.write_model(b, back) == size == os.path.getsize(a)
    assert open(a, "rb").read() == open(b, "rb").read()
    header = 4 + 44 + 8 + 4 * qm.filters.size + 4 + sum(4 + len(w) for w in qm.vocab)
    records = 0
    for name, shape, is_f16 in gf.tensor_specs(qm.hparams):
        n = int(np.prod(shape))
        t = qm.tensors[name]
        records += 12 + 4 * len(shape) + len(name) + (n // 32 * gf.BLOCK_BYTES[qtype] if isinstance(t, gf.QTensor) else n * (2 if is_f16 else 4))
    assert size == header + records
    assert gf.read_model(a, load_tensors=False).tensors == {}
    # smaller than the f16 file by what the blocks save
    assert size < gf.write_model(b, small_model)


def test_reader_refuses_what_it_cannot_read(small_model, tmp_path):
    qm = gf.quantize_model(small_model, "q5_0")
    path = str(tmp_path / "m.bin")
    gf.write_model(path, qm)
    image = bytearray(open(path, "rb").read())
    old = bytearray(image)
    old[4 + 40:4 + 44] = struct.pack("<i", 1008)                    # quantization version 1
    open(path, "wb").write(old)
    with pytest.raises(ValueError, match="quantization version is 1"):
        gf.read_model(path)
    # a record of type 4 (the removed q4_2): the first quantized record's type
    name = b"encoder.blocks.0.mlp.0.weight"
    at = image.index(name) - 8 - 12
    assert struct.unpack_from("<3i", image, at) == (2, len(name), 6)
    bad = bytearray(image)
    struct.pack_into("<i", bad, at + 8, 4)
    open(path, "wb").write(bad)
    with pytest.raises(ValueError, match="ggml type 4"):
        gf.read_model(path)
    open(path, "wb").write(image[:image.index(name) + len(name) + 3 * 22 + 5])         # inside the fourth block of that tensor
    with pytest.raises(ValueError, match="truncated"):
        gf.read_model(path)


def test_quantize_tool(small_model, tmp_path):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    gf.write_model(src, small_model)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "whisper_amd.quantize", src, dst, "q5_0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    want = str(tmp_path / "want.bin")
    gf.write_model(want, gf.quantize_model(gf.read_model(src), "q5_0"))
    assert open(dst, "rb").read() == open(want, "rb").read()
    assert subprocess.run([sys.executable, "-m", "whisper_amd.quantize", src, dst, "q6_k"], stderr=subprocess.PIPE, env=env, cwd=ROOT).returncode == 2
    assert subprocess.run([sys.executable, "-m", "whisper_amd.quantize", dst, src, "q4_0"], stderr=subprocess.PIPE, env=env, cwd=ROOT).returncode == 1


# ---------------------------------------------------------------------------------------------------------------------
# ggmlTensor.h through tests/quant_cpu/driver.cpp, a program of its own under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "quant-driver")
    src = os.path.join(ROOT, "tests", "quant_cpu", "driver.cpp")
    hdr = os.path.join(ROOT, "whisper_amd", "host", "ggmlTensor.h")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in (src, hdr)):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.dirname(hdr), src, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    return exe


def run_driver(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode in (0, 2), (r.returncode, r.stderr[-2000:])
    return r.returncode, r.stdout.strip()


def test_ggml_tensor_header(driver):
    # payload sizes per type, 1 to 3 dimensions
    per32 = {0: 128, 1: 64, 2: 18, 3: 20, 6: 22, 7: 24, 8: 34}
    for t, size in per32.items():
        for ne in ((32,), (128, 384), (1024, 51865), (64, 3, 5)):
            n = int(np.prod(ne))
            assert run_driver(driver, "payload", t, 2008, *ne) == (0, "ok %d %d" % (n, n // 32 * size)), (t, ne)
    assert run_driver(driver, "payload", 0, 0, 48, 7) == (0, "ok 336 1344") and run_driver(driver, "payload", 1, 1, 3, 80, 128) == (0, "ok 30720 61440")
    for t, name in ((2, "q4_0"), (3, "q4_1"), (6, "q5_0"), (7, "q5_1"), (8, "q8_0")):
        assert run_driver(driver, "block", t) == (0, "%d %s" % (per32[t], name))
    assert run_driver(driver, "block", 1)[1].split()[0] == "0"
    # types that are not read: by name and number
    for t, word in ((4, "q4_2"), (5, "q4_3"), (9, "q8_1"), (12, "q4_k"), (-1, "unknown"), (16, "unknown")):
        rc, out = run_driver(driver, "payload", t, 2008, 128, 128)
        assert rc == 2 and out.startswith("rejected: ") and ("type %d" % t) in out and word in out, out
    # rows that are not whole blocks (fine for f16)
    for t in (2, 3, 6, 7, 8):
        rc, out = run_driver(driver, "payload", t, 2008, 48, 64)
        assert rc == 2 and "48" in out and "32" in out, out
    assert run_driver(driver, "payload", 1, 1, 48, 64)[0] == 0
    # a product beyond int64, and one beyond 2^31 - 1 blocks; the largest that is accepted
    big = 2 ** 31 - 1
    for t in (0, 1, 8):
        rc, out = run_driver(driver, "payload", t, 2008, big - 30 if t == 8 else big, big, big)
        assert rc == 2 and "overflow" in out, out
    rc, out = run_driver(driver, "payload", 6, 2008, 2 ** 20, 2 ** 16)
    assert rc == 2 and "blocks" in out, out
    assert run_driver(driver, "payload", 6, 2008, 2 ** 20, 2 ** 16 - 1) == (0, "ok %d %d" % (2 ** 36 - 2 ** 20, (2 ** 31 - 2 ** 15) * 22))
    assert run_driver(driver, "payload", 0, 0, big, 2 ** 29) == (0, "ok %d %d" % (big * 2 ** 29, big * 2 ** 31))         # the bytes still fit int64
    for ne in ((0,), (32, -1), (32, 4, 0)):
        assert run_driver(driver, "payload", 1, 1, *ne)[0] == 2
    # quantized records want quantization version 2; f32 / f16 records ignore the field
    for f16 in (1008, 8, 1, 0, 3008):
        rc, out = run_driver(driver, "payload", 6, f16, 128, 128)
        assert rc == 2 and "version is %d" % (f16 // 1000) in out, out
        assert run_driver(driver, "payload", 1, f16, 128, 128)[0] == 0
    # the header's f16 field in numbers and in words
    assert run_driver(driver, "header", 2008) == (0, "2 8 q5_0, quantization version 2")
    assert run_driver(driver, "header", 1008) == (0, "1 8 q5_0, quantization version 1")
    assert run_driver(driver, "header", 8) == (0, "0 8 q5_0, quantization version 0")
    assert run_driver(driver, "header", 1) == (0, "0 1 f16")
    assert run_driver(driver, "header", 0) == (0, "0 0 f32")
    assert run_driver(driver, "header", 2007) == (0, "2 7 q8_0, quantization version 2")
    assert run_driver(driver, "header", 2002)[1] == "2 2 q4_0, quantization version 2" and run_driver(driver, "header", 2003)[1].startswith("2 3 q4_1")
    assert run_driver(driver, "header", 2009)[1].startswith("2 9 q5_1")
