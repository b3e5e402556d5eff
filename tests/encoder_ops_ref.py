"""Plain numpy restatements of the encoder's four fused products and of the layout of conv1's operand -- TEST INFRASTRUCTURE ONLY.

What wh_encode builds by hand (whisper_amd/csrc/encode.hip) and wh_op_gemm_encoder exposes, restated from the comments there and from epilogueOne
(csrc/epilogue.h), with explicit slicing and loops over windows instead of the kernels' address arithmetic:

  mel -> conv input   x16[b][t + 1][c] = fp16( mel_b[c][off_b + t] ), zero beyond the spectrogram, rows 0 and rows + 1 untouched
  conv1               row t of window b = padded rows t, t + 1, t + 2 side by side (k = 3, stride 1); GELU; written to padded row t + 1
  conv2               row t = padded rows 2 t, 2 t + 1, 2 t + 2 (stride 2); GELU; + positional row t
  Q/K/V               head split; V of a (window, head) in the operand order of the attention's P.V matrix instruction (v_frag_index)
  cross-K/V           [layer][B][head][T][64] with the chunk's first window at an offset; K scaled, V biased

Products are formed in float64. With the inputs of dyadic() every product is a multiple of 2^-7 and every partial sum of K <= 1280 terms stays below 2^12, that is
19 significant bits: ANY order of summation in FP32 gives the float64 sum exactly (tests/test_encoder_ops_ref_cpu.py proves it on the largest K), so the accumulator
the epilogue sees is known bit for bit. What follows the sum is a fixed sequence of single FP32 operations and FP16 roundings, repeated here in np.float32 /
np.float16 in epilogueOne's order. Outputs are returned as bit patterns (uint16 / float32 viewed as uint32 by the caller) in buffers pre-filled with a sentinel, so that
"every live element equals, everything else untouched" is one array comparison.
"""
import numpy as np

HEAD_DIM = 64
SENTINEL16 = np.uint16(0x7BFF)            # FP16 65504: never produced by the inputs used here
SENTINEL32 = np.uint32(0x7FC0BEEF)        # an FP32 NaN with a payload


def round_up(x, m):
    return (x + m - 1) // m * m


def v_frag_index(key, dd):
    """csrc/epilogue.h vFragIndex: where element (key, dd) of a (window, head)'s V lies: blocks of 16 keys x 32 dims hold lane-major 8-half fragments."""
    key, dd = np.asarray(key, np.int64), np.asarray(dd, np.int64)
    return (((key >> 4) * 2 + (dd >> 5)) * 64 + ((key >> 2) & 1) * 32 + (dd & 31)) * 8 + ((key >> 3) & 1) * 4 + (key & 3)


def dyadic(rng, shape, step, lim):
    """Multiples of `step` (a power of two) in [-lim, lim], as float64."""
    n = int(round(lim / step))
    return rng.integers(-n, n + 1, size=shape).astype(np.float64) * step


def activations(rng, shape):
    return dyadic(rng, shape, 1.0 / 8, 2.0).astype(np.float16)


def weights(rng, shape):
    return dyadic(rng, shape, 1.0 / 16, 1.0).astype(np.float16)


def biases(rng, shape):
    return dyadic(rng, shape, 1.0 / 128, 4.0).astype(np.float32)


# ---- operand layouts ------------------------------------------------------------------------------------------------------------------------------
def conv_weight_rows(w_file, kpad):
    """csrc/model.hip: a convolution weight of the file, [out][in][3] (tap contiguous), as the rows of the implicit GEMM: [out][tap * in + c], zero padded to kpad."""
    oc, ic, taps = w_file.shape
    assert taps == 3 and kpad >= 3 * ic
    rows = np.zeros((oc, kpad), w_file.dtype)
    for tap in range(3):
        rows[:, tap * ic:(tap + 1) * ic] = w_file[:, :, tap]
    return rows


def mel_to_conv_input(mels, offsets, n_mels, rows, stride=None):
    """mels[b]: FP32 [n_mels][len_b] or None (a silent window). Returns uint16 [batch][stride], stride >= (rows + 2) * n_mels, sentinel where nothing is written."""
    stride = (rows + 2) * n_mels if stride is None else stride
    out = np.full((len(mels), stride), SENTINEL16, np.uint16)
    for b, (mel, off) in enumerate(zip(mels, offsets)):
        body = np.zeros((rows, n_mels), np.float32)
        if mel is not None:
            have = max(0, min(rows, mel.shape[1] - off))
            body[:have] = mel[:, off:off + have].T
        out[b, n_mels:(rows + 1) * n_mels] = body.astype(np.float16).view(np.uint16).reshape(-1)
    return out


# ---- accumulators (float64) ------------------------------------------------------------------------------------------------------------------------
def conv_acc(xpad, w_rows, stride):
    """xpad: FP16 [batch][Tin + 2][ic] (rows 0 and Tin + 1 are the zero padding); w_rows: FP16 [oc][kpad] as conv_weight_rows. Output row t of a window is the dot
    product of padded rows stride * t + (0, 1, 2), laid side by side, with the first 3 * ic columns of each weight row -> float64 [batch][Tin / stride][oc]."""
    batch, tp, ic = xpad.shape
    n_out = (tp - 2) // stride
    w = w_rows[:, :3 * ic].astype(np.float64)
    out = np.empty((batch, n_out, w_rows.shape[0]), np.float64)
    step = max(1, 16384 // n_out)                                # windows per product: a few thousand rows of the im2col matrix at a time
    for b in range(0, batch, step):
        x = xpad[b:b + step].astype(np.float64)
        col = np.concatenate([x[:, tap:tap + stride * n_out:stride][:, :n_out] for tap in range(3)], axis=2)      # im2col by slicing: [windows][n_out][3 ic]
        out[b:b + step] = col @ w.T
    return out


def mul_acc(a, w):
    """a: FP16 [M][K], w: FP16 [N][K] -> float64 [M][N]."""
    return a.astype(np.float64) @ w.astype(np.float64).T


def as_f32_exact(acc):
    """The FP32 accumulator of an exact sum: the float64 value must be representable."""
    a32 = acc.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), acc), "the sum is not representable in FP32: the inputs are outside dyadic()'s contract"
    return a32


# ---- epilogues (epilogueOne's arithmetic, FP32 / FP16 step by step) ----------------------------------------------------------------------------------
def gelu_arg_bits(acc32, bias):
    """The FP16 bit pattern gelu16 looks at: fp16( acc + bias[n] ), one FP32 addition, one rounding."""
    return (acc32 + np.asarray(bias, np.float32).reshape(-1)).astype(np.float32).astype(np.float16).view(np.uint16)


def epi_conv1(acc32, bias, gelu_map):
    """EPI_F16_GELU into the padded time-major buffer of conv2's operand: acc32 [batch][Mb][d] -> uint16 [batch][Mb + 2][d], rows 0 and Mb + 1 sentinel."""
    batch, mb, d = acc32.shape
    out = np.full((batch, mb + 2, d), SENTINEL16, np.uint16)
    out[:, 1:mb + 1] = gelu_map[gelu_arg_bits(acc32, bias)]
    return out


def epi_conv2(acc32, bias, pe, gelu_map):
    """EPI_CONV2: acc32 [batch][T][d], pe FP32 [T][d] -> FP32 [batch * T][d] = pe[t] + float( gelu16( acc + bias ) )."""
    batch, T, d = acc32.shape
    g = gelu_map[gelu_arg_bits(acc32, bias)].view(np.float16).astype(np.float32)
    return (pe[None, :T].astype(np.float32) + g).astype(np.float32).reshape(batch * T, d)


def epi_qkv(acc32, bias, H, Tpad):
    """EPI_QKV_ENC: acc32 [batch][T][3 d] -> q, k uint16 [batch][H][T][64], v uint16 [batch][H][64 * Tpad] (sentinel where no key lives)."""
    batch, T, n = acc32.shape
    d = H * HEAD_DIM
    assert n == 3 * d and Tpad >= round_up(T, 16)
    x = (acc32 + np.asarray(bias, np.float32).reshape(-1)).astype(np.float32).astype(np.float16).view(np.uint16)
    q = np.empty((batch, H, T, HEAD_DIM), np.uint16)
    k = np.empty((batch, H, T, HEAD_DIM), np.uint16)
    v = np.full((batch, H, HEAD_DIM * Tpad), SENTINEL16, np.uint16)
    key, dd = np.meshgrid(np.arange(T), np.arange(HEAD_DIM), indexing="ij")
    idx = v_frag_index(key, dd)
    for h in range(H):
        q[:, h] = x[:, :, h * 64:(h + 1) * 64]
        k[:, h] = x[:, :, d + h * 64:d + (h + 1) * 64]
        v[:, h][:, idx.ravel()] = x[:, :, 2 * d + h * 64:2 * d + (h + 1) * 64].reshape(batch, T * HEAD_DIM)
    return q, k, v


def epi_cross(acc32, bias, scale, H, B, b0):
    """EPI_CROSS_KV: acc32 [batch][T][layers * 2 d] -> k, v uint16 [layers][B][H][T][64] with the batch at windows b0 .. b0 + batch - 1, sentinel elsewhere;
    k = fp16( acc * scale ), v = fp16( acc + bias )."""
    batch, T, n = acc32.shape
    d = H * HEAD_DIM
    layers = n // (2 * d)
    assert n == layers * 2 * d and b0 + batch <= B
    k = np.full((layers, B, H, T, HEAD_DIM), SENTINEL16, np.uint16)
    v = np.full((layers, B, H, T, HEAD_DIM), SENTINEL16, np.uint16)
    kb = (acc32 * np.float32(scale)).astype(np.float32).astype(np.float16).view(np.uint16)
    vb = (acc32 + np.asarray(bias, np.float32).reshape(-1)).astype(np.float32).astype(np.float16).view(np.uint16)
    for layer in range(layers):
        for h in range(H):
            c = layer * 2 * d + h * 64
            k[layer, b0:b0 + batch, h] = kb[:, :, c:c + 64]
            v[layer, b0:b0 + batch, h] = vb[:, :, c + d:c + d + 64]
    return k, v


def f16_ulp_distance(a_bits, b_bits):
    """Distance in FP16 units in the last place between two arrays of finite FP16 bit patterns (sign-magnitude -> a monotone integer line)."""
    def line(u):
        u = u.astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u)
    return np.abs(line(a_bits) - line(b_bits))
