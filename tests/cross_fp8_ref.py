"""The format of the FP8 cross-attention caches (whisper_amd/csrc/kv8.hip), stated in numpy: rows of 64 FP16 values -> OCP E4M3 bytes and one power-of-two
scale per row, s = 2^ceil( log2( amax / 448 ) ), 1 for a row of zeros; the bytes are x / s (exact) rounded to E4M3, to nearest even (torch.float8_e4m3fn)."""
import numpy as np
import torch


def quantize_rows(x16):
    """x16 [..., 64] float16 -> (bytes uint8 [..., 64], scales float32 [...])."""
    x = np.asarray(x16, np.float16).astype(np.float64)
    amax = np.abs(x).max(axis=-1)
    m, e = np.frexp(amax)                                  # amax = m 2^e, 0.5 <= m < 1; 448 = 0.875 * 2^9: the smallest s = 2^k with 448 s >= amax
    s = np.where(amax > 0, np.ldexp(1.0, e - 9 + (m > 0.875)), 1.0)
    y = torch.from_numpy((x / s[..., None]).astype(np.float32)).to(torch.float8_e4m3fn)
    return y.view(torch.uint8).numpy(), s.astype(np.float32)


def dequantize(b, s):
    """bytes [..., 64], scales [...] -> float64 [..., 64]: exact."""
    v = torch.from_numpy(np.ascontiguousarray(b)).view(torch.float8_e4m3fn).to(torch.float32).numpy().astype(np.float64)
    return v * np.asarray(s, np.float64)[..., None]
