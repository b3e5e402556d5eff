"""The format of the INT4 cross-attention caches (whisper_amd/csrc/kv4.hip), stated in numpy -- TEST INFRASTRUCTURE ONLY.

  codes   per key row of 64 FP16 values: amax = max |x|, s = amax / 7 in FP32 (1 for a row of zeros), n = rint( x / s ) to nearest even with FP32 division,
          clipped to [-7, 7]; the nibble stored is n + 8 (1 .. 15, never 0). One FP32 scale per row; K and V by the same rule.
  K       [..., T, 32] bytes: byte t of a row = nibble of dim 2 t | nibble of dim 2 t + 1 << 4.
  V       [..., ceil( T / 64 ), 64 dims, 32] bytes: blocks of 64 keys, dim-major inside a block; a dim's 32 bytes are 8 words of 8 keys, byte t of word w =
          nibble of key 8 w + t | nibble of key 8 w + 4 + t << 4. Keys behind T inside the last block: nibble 0.

Run as a script it predicts, on the CPU, how far these caches move the logits of the d = 128 test model:  python tests/cross_i4_ref.py
"""
import numpy as np

F32 = np.float32


def quantize(x16):
    """x16 [..., 64] float16 -> (codes int8 [..., 64] in [-7, 7], scales float32 [...])."""
    x = np.asarray(x16, np.float16).astype(F32)
    amax = np.abs(x).max(axis=-1)
    s = np.where(amax > 0, amax / F32(7), F32(1)).astype(F32)
    return np.clip(np.rint((x / s[..., None]).astype(F32)), -7, 7).astype(np.int8), s


def dequantize(n, s):
    """codes [..., 64], scales [...] -> float64 [..., 64]: exact."""
    return n.astype(np.float64) * np.asarray(s, np.float64)[..., None]


def pack_k(n):
    """codes [..., T, 64] -> bytes [..., T, 32]."""
    u = (n.astype(np.int16) + 8).astype(np.uint8)
    return u[..., 0::2] | (u[..., 1::2] << 4)


def unpack_k(b):
    u = np.stack([b & 15, b >> 4], axis=-1).reshape(b.shape[:-1] + (64,))
    return u.astype(np.int8) - 8


def pack_v(n):
    """codes [..., T, 64] -> bytes [..., ceil( T / 64 ), 64, 32]."""
    T = n.shape[-2]
    kb = (T + 63) // 64
    u = np.zeros(n.shape[:-2] + (kb * 64, 64), np.uint8)
    u[..., :T, :] = (n.astype(np.int16) + 8).astype(np.uint8)
    u = np.swapaxes(u.reshape(n.shape[:-2] + (kb, 64, 64)), -1, -2)            # [..., block, dim, key]
    u = u.reshape(u.shape[:-1] + (8, 2, 4))                                    # key = 8 w + 4 half + t
    return (u[..., 0, :] | (u[..., 1, :] << 4)).reshape(n.shape[:-2] + (kb, 64, 32))


def unpack_v(b, T):
    """bytes [..., blocks, 64, 32] -> codes [..., T, 64]; the padding keys of the last block are dropped."""
    w = b.reshape(b.shape[:-1] + (8, 4))
    u = np.stack([w & 15, w >> 4], axis=-2).reshape(b.shape[:-1] + (64,))      # [..., block, dim, key]
    u = np.swapaxes(u, -1, -2).reshape(b.shape[:-3] + (b.shape[-3] * 64, 64))
    return u[..., :T, :].astype(np.int8) - 8


def measure_logit_shift():
    """Largest |logit( INT4 caches ) - logit( FP16 caches )| of oracle/whisper_np.py on the d = 128 test model: the prompt step plus 3 steps of 3 windows, the
    inputs of tests/test_gpu_cross_i4.py::test_decode_steps_against_the_fp16_context. The caches are replaced by their dequantized codes (FP32)."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from oracle import whisper_np as wn
    from whisper_amd import ggml_format as gf
    model = gf.synth_model("test-d128", seed=1234, attn_sharpness=2.0)
    hp = model.hparams
    gmel = np.load(os.path.join(root, "tests", "golden", "ref_test_d128.npz"))["mel"]
    rng = np.random.default_rng(5)
    mels = np.stack([np.roll(gmel, 37 * b, axis=1) + 0.01 * rng.standard_normal(gmel.shape).astype(F32) for b in range(3)]).astype(F32)
    sp = gf.special_tokens(hp)
    steps = [[[sp["sot"], sp["transcribe"], sp["not_"]]] * 3] + [[[100 + 7 * i + b] for b in range(3)] for i in range(3)]
    worst = 0.0
    for b in range(3):
        logits = []
        for i4 in (False, True):
            net = wn.WhisperNP(model)
            net.encode(mels[b])
            if i4:
                for cache in (net.kv.cross_k, net.kv.cross_v):
                    for il, c in enumerate(cache):
                        rows = np.asarray(c, F32).reshape(c.shape[0], -1, 64)
                        cache[il] = dequantize(*quantize(rows.astype(np.float16))).reshape(c.shape).astype(F32)
            n_past, out = 0, []
            for t in steps:
                out.append(np.asarray(net.decode(t[b], n_past, exact_pv=False)[0], F32)[-1])   # the last token's row, P.V not in the CPU path's FP16 steps: what wh_decode computes
                n_past += len(t[b])
            logits.append(out)
        worst = max(worst, max(float(np.abs(a - c).max()) for a, c in zip(*logits)))
    return worst


if __name__ == "__main__":
    print("max |d logit|, INT4 cross-attention caches against FP16, whisper_np on test-d128: %.4e" % measure_logit_shift())
