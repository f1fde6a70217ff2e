#!/usr/bin/env python3
"""Re-pack a checkpoint converted by tools/import_keras_hdf5.py so that it fits the 1 MiB limit of a committed fixture.

    python tools/pack_keras_npz.py <in.npz> <out.npz> [--quantize]

Always: the same arrays, re-written as a zip with LZMA members (np.load reads them as it reads any .npz).
--quantize: additionally replaces the latent float kernels of BinaryConv2D / BinaryDense / TernaryConv2D /
TernaryDense layers by their quantized values binarize(W, H) / ternarize(W, H).  Both quantizers are idempotent
(binarize(+-H) = +-H; ternarizing t * H again gives a cutoff 0.7 * mean|t| < 1, so +-1 and 0 stay put), so every
forward pass -- engine and oracle alike -- computes exactly what it computes on the original checkpoint, and the
kernels compress to a few bits per weight.
"""
import argparse
import io
import json
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import qnn_oracle as O  # noqa: E402

_QUANTIZE = {"BinaryConv2D": O.binarize, "BinaryDense": O.binarize,
             "TernaryConv2D": O._ternarize, "TernaryDense": O._ternarize}


def pack(src, dst, quantize=False):
    d = dict(np.load(src))
    if quantize:
        cfg = json.loads(bytes(d["model_config_json"]).decode())
        for l in cfg["config"]["layers"]:
            f = _QUANTIZE.get(l["class_name"])
            if f is not None:
                key = l["name"] + "/kernel"
                d[key] = np.asarray(f(d[key], float(l["config"].get("H", 1.0))), dtype=np.float32)
                assert np.array_equal(f(d[key], float(l["config"].get("H", 1.0))), d[key]), key
    with zipfile.ZipFile(dst, "w", compression=zipfile.ZIP_LZMA) as z:
        for k, v in d.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(v), allow_pickle=False)
            z.writestr(k + ".npy", buf.getvalue())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--quantize", action="store_true")
    a = ap.parse_args()
    pack(a.src, a.dst, a.quantize)
    print("wrote %s (%d bytes)" % (a.dst, os.path.getsize(a.dst)))
