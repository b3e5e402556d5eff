"""Quantize a ggml Whisper model file: the counterpart of whisper.cpp's `quantize` tool. CPU only.

    python -m whisper_amd.quantize in.bin out.bin q5_0        # q4_0, q4_1, q5_0, q5_1 or q8_0

The 2-D `*.weight` matrices (the linear layers and the token embedding) become blocks of 32 elements, everything else is copied, and the
header's f16 field becomes 2000 + ftype (ggml_format.quantize_model). The loaders expand such a file on the device into the FP16 arena
of its dequantized values (ggml_format.dequantized_twin is the f16 file that loads to the same bytes).
"""
from __future__ import annotations

import os
import sys

from . import ggml_format as gf


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) != 3 or argv[2] not in gf.GGML_TYPES:
        sys.stderr.write("usage: python -m whisper_amd.quantize in.bin out.bin {%s}\n" % "|".join(sorted(gf.GGML_TYPES)))
        return 2
    src, dst, qtype = argv
    model = gf.read_model(src)
    if any(isinstance(a, gf.QTensor) for a in model.tensors.values()):
        sys.stderr.write("%s is quantized already\n" % src)
        return 1
    out = gf.quantize_model(model, qtype)
    size = gf.write_model(dst, out)
    n = sum(isinstance(a, gf.QTensor) for a in out.tensors.values())
    print("%s: %d of %d tensors as %s, %.1f MB -> %.1f MB" % (dst, n, len(out.tensors), qtype, os.path.getsize(src) / 1e6, size / 1e6))
    return 0


if __name__ == "__main__":
    sys.exit(main())
