"""The format and the product of the INT8 encoder path (whisper_amd/csrc/quant_i8.hip, gemm_i8.hip), stated in numpy -- TEST INFRASTRUCTURE ONLY.

  rows      symmetric int8, one FP32 scale per row of K values: amax = max |x| over the row's FP16 values, s = amax / 127 in FP32 (1 for a row of zeros),
            q = rint( x / s ) to nearest even with FP32 division, clamped to [-127, 127]. Weights [N][K] by the same rule per output row.
  product   acc = sum_k qa[m][k] qw[n][k], exact (a float64 matmul: |acc| <= 127^2 K < 2^53); y = ( float32( acc ) * sa[m] ) * sw[n], every step one FP32 rounding;
            then epilogueOne's arithmetic on y (encoder_ops_ref.py).

Run as a script it measures, on the CPU, how far the INT8 products move the logits of the d = 128 test model (the constant E of tests/test_gpu_encoder_i8.py and
DESIGN.md section 7):  python tests/encoder_i8_ref.py
"""
import numpy as np

F32 = np.float32


def quantize_rows(x16):
    """x16 [..., K] float16 -> (q int8 [..., K], s float32 [...])."""
    x = np.asarray(x16, np.float16).astype(F32)
    amax = np.abs(x).max(axis=-1)
    s = np.where(amax > 0, amax / F32(127), F32(1)).astype(F32)
    q = np.clip(np.rint((x / s[..., None]).astype(F32)), -127, 127)
    return q.astype(np.int8), s


def product(qa, sa, qw, sw):
    """y float32 [M][N] = ( float32( qa . qw^T ) * sa[m] ) * sw[n]."""
    acc = qa.astype(np.float64) @ qw.astype(np.float64).T
    return ((acc.astype(F32) * sa[:, None]).astype(F32) * sw[None, :]).astype(F32)


def mul_mat(w16, x):
    """The INT8 restatement in the place of whisper_np.mul_mat_w: FP16 weight [out][in], FP32 activations [rows][in] rounded to FP16 first."""
    qa, sa = quantize_rows(np.asarray(x, F32).astype(np.float16))
    qw, sw = quantize_rows(w16)
    return product(qa, sa, qw, sw)


def measure_logit_shift():
    """Largest |logit( encoder with INT8 products ) - logit( FP16 encoder )| of oracle/whisper_np.py on the d = 128 test model: the prompt step plus 3 steps of 3
    windows, the inputs of tests/test_gpu_cross_fp8.py::test_decode_steps_against_the_fp16_context. The four encoder weight families go through mul_mat, everything
    else (convolutions, cross-K/V, decoder) stays as it is."""
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
    enc = {id(w) for name, w in model.tensors.items() if name.startswith("encoder.blocks.") and name.endswith(".weight") and (".attn." in name or ".mlp." in name)}
    assert len(enc) == 6 * hp.n_audio_layer
    plain = wn.mul_mat_w
    worst = 0.0
    for b in range(3):
        logits = []
        for i8 in (False, True):
            wn.mul_mat_w = (lambda w16, x: mul_mat(w16, x) if id(w16) in enc else plain(w16, x)) if i8 else plain
            try:
                net = wn.WhisperNP(model)
                net.encode(mels[b])
            finally:
                wn.mul_mat_w = plain
            n_past, out = 0, []
            for t in steps:
                out.append(np.asarray(net.decode(t[b], n_past)[0], F32))
                n_past += len(t[b])
            logits.append(out)
        worst = max(worst, max(float(np.abs(a - c).max()) for a, c in zip(*logits)))
    return worst


if __name__ == "__main__":
    print("max |d logit|, INT8 encoder products against FP16, whisper_np on test-d128: %.4e" % measure_logit_shift())
