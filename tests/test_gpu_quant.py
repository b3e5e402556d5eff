"""GPU tests of the quantized ggml models: the dequantization kernel (whisper_amd/csrc/dequant.hip; wh_dequantize of include/whisper_hip.h), the loader
behind it (wh_model_set_tensor with a quantized type) and what sits on top: HipModel.from_ggml, api.Model (libWhisper.so: loadGgmlFile) and whisper-main.

The contract is exact: a quantized matrix is loaded as the FP16 matrix of fp16( (float)d * (float)( q - off ) ) resp. fp16( (float)d * (float)q + (float)m ),
so everything is compared bit for bit -- the kernel with the numpy restatement (ggml_format.dequantize_f16; NaN as NaN), the arena of a quantized model with the
arena of its F16 twin, the transcripts of the two files with ==. No tolerance anywhere.
Sources sit inside larger device buffers of 0xFF bytes, destinations inside buffers of FP16 NaN whose bytes around the destination must not change."""
import ctypes as C
import importlib.util
import os
import struct
import subprocess
import wave

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from whisper_amd import api, binding, build, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ("q4_0", "q4_1", "q5_0", "q5_1", "q8_0")
SPAN = 256                  # blocks per workgroup of dequantKernel
COUNTS = (1, 2, 63, 64, 65, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 1, 65537)
GUARD = 128                 # bytes on both sides of a source and of a destination: keeps the 16-byte alignment
INVALID = -1                # WH_E_INVALIDARG
NAN16 = 0x7E00


def half_bytes(bits):
    return np.asarray(bits, np.uint16).astype("<u2").view(np.uint8).reshape(-1, 2)


def edge_blocks(qtype, rng):
    """Blocks [n][blockBytes] that random bytes rarely give: every nibble and qh pattern, the special scales, the int8 extremes, sums that cancel"""
    size = gf.BLOCK_BYTES[qtype]
    has_m, five = qtype.endswith("_1"), qtype.startswith("q5")
    qs_at = 2 + 2 * has_m + 4 * five
    rows = []

    def block(d_bits, m_bits=0x3800, qh=0, qs=None):
        b = np.zeros(size, np.uint8)
        b[0:2] = half_bytes([d_bits])[0]
        if has_m:
            b[2:4] = half_bytes([m_bits])[0]
        if five:
            b[qs_at - 4:qs_at] = np.frombuffer(struct.pack("<I", qh & 0xFFFFFFFF), np.uint8)
        b[qs_at:] = rng.integers(0, 256, size - qs_at, dtype=np.uint8) if qs is None else qs
        rows.append(b)

    n_qs = size - qs_at
    # every byte value -- every pair of nibbles resp. every int8 -- at every position of qs
    for v in range(256):
        block(0x3C00, qs=(v + 17 * np.arange(n_qs)) % 256)
    for v in range(0, 256, 17):
        block(0x3555, qs=np.full(n_qs, v))
    if five:
        for qh in [0, 0xFFFFFFFF, 0xAAAAAAAA, 0x55555555, 0x0000FFFF, 0xFFFF0000, 0x00FF00FF] + [1 << i for i in range(32)] + [~(1 << i) for i in range(0, 32, 5)]:
            block(0x3C00, qh=qh, qs=np.zeros(n_qs))
            block(0xB400, qh=qh)
    # d: 0, -0, the smallest and the largest subnormal, 65504, inf, NaN, and their negatives; m the same where the type has one
    special = [0x0000, 0x8000, 0x0001, 0x03FF, 0x7BFF, 0x7C00, 0x7E00, 0x8001, 0x83FF, 0xFBFF, 0xFC00, 0x0400, 0x7C01]
    for d in special:
        block(d)
        block(d, qs=np.zeros(n_qs))
        block(d, qh=0xFFFFFFFF, qs=np.full(n_qs, 0xFF))
        if has_m:
            for m in special:
                block(d, m_bits=m)
    if qtype == "q8_0":
        for d in (0x3C00, 0x7BFF, 0x0001, 0x5800):
            block(d, qs=np.full(32, 0x80))                     # -128
            block(d, qs=np.full(32, 0x7F))                     # 127
            block(d, qs=np.tile(np.asarray([0x80, 0x7F], np.uint8), 16))
    if has_m:
        # m = -15 d with d of seven significant bits, so that m is exact: q = 15 cancels to zero, its neighbours to +-d
        for _ in range(24):
            d_bits = int(rng.integers(0x0400, 0x6800)) & 0xFFF0
            d = np.asarray([d_bits], np.uint16).view(np.float16)[0]
            m_bits = int(np.asarray([-15.0 * float(d)], np.float32).astype(np.float16).view(np.uint16)[0])
            assert float(np.asarray([m_bits], np.uint16).view(np.float16)[0]) == -15.0 * float(d)
            block(d_bits, m_bits=m_bits, qh=0)
            block(d_bits, m_bits=m_bits, qh=0, qs=np.full(n_qs, 0xFF))
    return np.stack(rows)


POOL = {}


def pool(qtype):
    """max( COUNTS ) blocks -- the edge blocks spread over the first two workgroup spans, random bytes elsewhere -- and their FP16 values by the numpy
    restatement: built once per type, shared by the tests, left unchanged. Blocks are independent, so the first n blocks are the reference of a call of n."""
    if qtype not in POOL:
        rng = np.random.default_rng(100 + gf.GGML_TYPES[qtype])
        n = max(COUNTS)
        raw = rng.integers(0, 256, (n, gf.BLOCK_BYTES[qtype]), dtype=np.uint8)
        edges = edge_blocks(qtype, rng)
        # a few at the very front (the calls of 1 and 2 blocks), the rest after block 8 with random blocks in between, and again at the far end
        raw[0] = edges[0]
        raw[1] = edges[len(edges) // 2]
        at = 8 + np.sort(rng.choice(max(2 * SPAN, 2 * len(edges)), len(edges), replace=False))
        raw[at] = edges
        raw[n - len(edges):] = edges
        want = gf.dequantize_f16(gf.QTensor(qtype, (n, 32), raw)).view(np.uint16).reshape(n, 32)
        raw.setflags(write=False)
        want.setflags(write=False)
        POOL[qtype] = (raw, want, int(at.max()) + 1)
    return POOL[qtype]


def device_dequantize(qtype, raw, n, front=GUARD):
    """wh_dequantize on the first n blocks, placed `front` bytes into a buffer of 0xFF, into a destination surrounded by FP16 NaN that must stay"""
    size = gf.BLOCK_BYTES[qtype]
    host = np.full(front + n * size + GUARD, 0xFF, np.uint8)
    host[front:front + n * size] = raw[:n].reshape(-1)
    src = torch.from_numpy(host).cuda()
    dst = torch.full((GUARD // 2 + 32 * n + GUARD // 2,), NAN16, dtype=torch.int16, device="cuda")
    binding.check(binding.lib().wh_dequantize(None, gf.GGML_TYPES[qtype], C.c_void_p(src.data_ptr() + front), n, C.c_void_p(dst.data_ptr() + GUARD)))
    torch.cuda.synchronize()
    out = dst.cpu().numpy().view(np.uint16)
    assert (out[:GUARD // 2] == NAN16).all() and (out[GUARD // 2 + 32 * n:] == NAN16).all(), "write outside the destination"
    assert torch.equal(src.cpu(), torch.from_numpy(host)), "the source was written"
    return out[GUARD // 2:GUARD // 2 + 32 * n].reshape(n, 32).copy()


def assert_same_halves(got, want, what):
    g, w = got.view(np.float16), want.view(np.float16)
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), (what, "NaN", np.argwhere(np.isnan(g) != nan)[:5])
    same = (got == want) | nan
    assert same.all(), (what, np.argwhere(~same)[:5], got[~same][:5], want[~same][:5])


# ---- 1. the kernel against the numpy restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("qtype", TYPES)
def test_dequantize_against_the_restatement(qtype):
    raw, want, edges_end = pool(qtype)
    w16 = want.view(np.float16)
    # the pool holds what the test is about: NaN, both infinities, subnormal results, both zeros
    assert np.isnan(w16).any() and (w16 == np.inf).any() and (w16 == -np.inf).any() and ((w16 != 0) & (np.abs(w16) < 6.2e-5)).any()
    assert (want == 0x8000).any() and (want == 0).any() and edges_end <= max(COUNTS)
    for n in COUNTS:
        assert_same_halves(device_dequantize(qtype, raw, n), want[:n], (qtype, n))
    # another 16-byte offset of the source, and a call that starts in the middle of the pool: a block's values do not depend on where it sits
    assert_same_halves(device_dequantize(qtype, raw, 300, front=GUARD + 16), want[:300], (qtype, "offset 16"))
    assert_same_halves(device_dequantize(qtype, raw[5:], SPAN + 7, front=GUARD + 48), want[5:5 + SPAN + 7], (qtype, "from block 5"))


def test_dequantize_refuses_bad_calls():
    lib = binding.lib()
    src = torch.full((4096,), 0x11, dtype=torch.uint8, device="cuda")
    dst = torch.full((4096,), NAN16, dtype=torch.int16, device="cuda")
    s, d = src.data_ptr(), dst.data_ptr()
    assert s % 16 == 0 and d % 16 == 0
    vp = C.c_void_p
    for t in (0, 1, 4, 5, 9, 10, -1, 99):                                       # not a quantized type
        assert lib.wh_dequantize(None, t, vp(s), 4, vp(d)) == INVALID, t
        assert b"type" in lib.wh_last_error()
    for t in (gf.GGML_TYPES[q] for q in TYPES):
        assert lib.wh_dequantize(None, t, vp(s), -1, vp(d)) == INVALID
        assert lib.wh_dequantize(None, t, vp(s), 2 ** 31, vp(d)) == INVALID
        assert lib.wh_dequantize(None, t, None, 4, vp(d)) == INVALID and lib.wh_dequantize(None, t, vp(s), 4, None) == INVALID
        for off in (1, 2, 4, 8, 18):                                            # the documented rule: both pointers 16-byte aligned
            assert lib.wh_dequantize(None, t, vp(s + off), 4, vp(d)) == INVALID, off
            assert lib.wh_dequantize(None, t, vp(s), 4, vp(d + off)) == INVALID, off
        assert b"16-byte" in lib.wh_last_error()
        assert lib.wh_dequantize(None, t, None, 0, None) == 0                   # nothing to do: nothing is touched
    torch.cuda.synchronize()
    assert (dst.cpu().numpy().view(np.uint16) == NAN16).all(), "a refused call launched"
    assert lib.wh_dequantize(None, 8, vp(s + 32), 4, vp(d + 64)) == 0           # the same buffers at aligned offsets are taken
    torch.cuda.synchronize()
    out = dst.cpu().numpy().view(np.uint16)
    assert (out[:32] == NAN16).all() and (out[32 + 128:] == NAN16).all() and (out[32:32 + 128] != NAN16).all()


# ---- 2. the arena of a quantized model is the arena of its F16 twin --------------------------------------------------------
@pytest.fixture(scope="module")
def small_model():
    return gf.synth_model("test-d128", seed=31)


def load_into_arena(model):
    n = binding.arena_bytes(model.hparams)
    arena = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    hm = binding.HipModel.from_ggml(model, arena.data_ptr(), keepalive=arena)
    assert hm.arena() == (arena.data_ptr(), n)
    hm.close()
    torch.cuda.synchronize()
    return arena


@pytest.mark.parametrize("qtype", TYPES)
def test_arena_of_a_quantized_model_is_the_arena_of_its_twin(small_model, qtype):
    qm = gf.quantize_model(small_model, qtype)
    twin = gf.dequantized_twin(qm)
    a, b = load_into_arena(qm), load_into_arena(twin)
    assert torch.equal(a, b)
    # and it is not the unquantized model's: the comparison above compares something
    assert not torch.equal(a, load_into_arena(small_model))


def test_set_tensor_refuses_quantized_data_where_no_matrix_lives(small_model):
    """Only the plain FP16 matrices take blocks: a positional embedding (2-D, FP32 in the arena), a LayerNorm vector and a bias are refused by name, and so
    is a type number that is no type; the model loads afterwards as if nothing had happened."""
    hm = binding.HipModel(small_model.hparams)
    L = binding.lib()
    d = small_model.hparams.n_audio_state

    def rc_for(name, shape, type_id, nbytes):
        ne = (C.c_int32 * len(shape))(*reversed(shape))
        data = np.zeros(nbytes, np.uint8)
        return L.wh_model_set_tensor(hm.handle, name.encode(), len(shape), ne, type_id, data.ctypes.data_as(C.c_void_p))

    for name, shape in (("decoder.positional_embedding", (small_model.hparams.n_text_ctx, d)), ("decoder.ln.weight", (d,)),
                        ("encoder.blocks.0.mlp.0.bias", (4 * d,)), ("encoder.conv2.weight", (d, d, 3))):
        n = int(np.prod(shape))
        assert rc_for(name, shape, 6, n // 32 * 22 + 22) == INVALID
        msg = L.wh_last_error().decode()
        assert name in msg and "q5_0" in msg, msg
    for type_id, word in ((4, "q4_2"), (9, "q8_1"), (12, "q4_k"), (77, "unknown")):
        assert rc_for("encoder.blocks.0.mlp.0.weight", (4 * d, d), type_id, 4 * d * d * 2) == INVALID
        msg = L.wh_last_error().decode()
        assert "encoder.blocks.0.mlp.0.weight" in msg and str(type_id) in msg and word in msg, msg
    hm.close()


# ---- 3. through the product ------------------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_runfull", os.path.join(ROOT, "tests", "golden", "make_golden_runfull.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def strip(segs):
    return [(s["t0"], s["t1"], s["text"], [t["id"] for t in s["tokens"]], [t["p"] for t in s["tokens"]]) for s in segs]


@pytest.fixture(scope="module")
def product_files(tmp_path_factory):
    """A conditioned multilingual test-d128 model (its tokens and timestamps depend on the audio) as a q5_0 file and as its F16 twin"""
    mg = _generator()
    tmp = tmp_path_factory.mktemp("quant")
    qm = gf.quantize_model(mg.model_for(10), "q5_0")
    q_path, twin_path = str(tmp / "cond-q5_0.bin"), str(tmp / "cond-twin.bin")
    gf.write_model(q_path, qm)
    gf.write_model(twin_path, gf.dequantized_twin(qm))
    return dict(q=q_path, twin=twin_path, pcm=mg.pcm_for("jfk"), dir=tmp)


def run_one(path, pcm):
    m = api.Model(path)
    ctx = m.create_context()
    assert ctx.run_full(pcm, language="en", flags=api.NO_CONTEXT) == 0
    res = strip(ctx.results())
    ctx.close()
    m.close()
    return res


def test_quantized_file_through_the_host_api(product_files):
    """api.Model goes through libWhisper.so and loadGgmlFile: the q5_0 file and its twin give the same segments -- ids, times and probabilities with =="""
    assert os.path.getsize(product_files["q"]) < os.path.getsize(product_files["twin"])
    got = run_one(product_files["q"], product_files["pcm"])
    want = run_one(product_files["twin"], product_files["pcm"])
    assert got == want and len(want) >= 1 and sum(len(s[3]) for s in want) >= 2


def test_quantized_file_through_whisper_main(product_files):
    assert os.path.exists(build.CLI_BIN)
    wav = str(product_files["dir"] / "jfk.wav")
    with wave.open(wav, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.clip(np.round(product_files["pcm"] * 32768.0), -32768, 32767).astype("<i2").tobytes())
    outs = []
    for key in ("q", "twin"):
        r = subprocess.run([build.CLI_BIN, "-m", product_files[key], "-f", wav, "-l", "en", "-nc"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1] and len(outs[0].strip()) > 0


def record_at(image, name):
    """(offset of the record, n_dims, type, offset of the payload) of tensor `name` in a file image"""
    nm = name.encode()
    at = image.index(nm)
    for n_dims in (1, 2, 3):
        head = at - 4 * n_dims - 12
        if struct.unpack_from("<2i", image, head) == (n_dims, len(nm)):
            return head, n_dims, struct.unpack_from("<i", image, head + 8)[0], at + len(nm)
    raise AssertionError(name)


def with_quantized_record(image, name, elements, old_bytes_per_element):
    """the image with tensor `name` stored as q5_0 blocks of zeros"""
    head, n_dims, _, payload = record_at(image, name)
    out = bytearray(image[:payload]) + bytes(elements // 32 * 22) + image[payload + elements * old_bytes_per_element:]
    struct.pack_into("<i", out, head + 8, 6)
    return out


def test_host_api_refuses_files_it_cannot_load(product_files, capfd):
    """Each broken file raises, the log says which tensor, which type and why, and the next F16 load in the same process works"""
    q = bytearray(open(product_files["q"], "rb").read())
    twin = bytearray(open(product_files["twin"], "rb").read())
    hp = gf.read_model(product_files["q"], load_tensors=False).hparams
    d, mels = hp.n_audio_state, hp.n_mels
    first_q = "encoder.blocks.0.mlp.0.weight"
    head, _, type_id, payload = record_at(q, first_q)
    assert type_id == 6

    v1 = bytearray(q)
    struct.pack_into("<i", v1, 4 + 40, 1008)
    removed = bytearray(q)
    struct.pack_into("<i", removed, head + 8, 4)
    as_2000 = bytearray(twin)                                                   # a quantized conv weight: its rows of 3 taps are no blocks
    struct.pack_into("<i", as_2000, 4 + 40, 2008)
    cases = {
        "version 1": (v1, [first_q, "q5_0", "quantization version is 1"]),
        "type 4": (removed, [first_q, "type 4", "q4_2"]),
        "conv1": (with_quantized_record(as_2000, "encoder.conv1.weight", d * mels * 3, 2), ["encoder.conv1.weight", "q5_0"]),
        "ln": (with_quantized_record(as_2000, "decoder.ln.weight", d, 4), ["decoder.ln.weight", "q5_0", "quantized"]),
        "truncated": (q[:payload + 3 * 22 + 5], [first_q, "truncated"]),
    }
    capfd.readouterr()
    for what, (image, words) in cases.items():
        path = str(product_files["dir"] / ("bad-%s.bin" % what.replace(" ", "-")))
        with open(path, "wb") as f:
            f.write(image)
        with pytest.raises(api.WhisperError):
            api.Model(path)
        err = capfd.readouterr().err
        for w in words:
            assert w in err, (what, w, err[-1500:])
        m = api.Model(product_files["twin"])                                    # nothing is left behind: the twin loads
        assert m.is_multilingual()
        m.close()
    assert run_one(product_files["q"], product_files["pcm"][:5 * 16000]) == run_one(product_files["twin"], product_files["pcm"][:5 * 16000])
