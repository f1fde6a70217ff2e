"""Time a 3x3 'same' stride-1 depthwise layer on int4 codes (4-bit weights, BN + quantized_tanh(4) to int4) two ways
(profiles/depthwise/README.md):

  depthwise  qnn_depthwise_forward (depthwise_i4, the 16-bit-lane form);
  expanded   what the parent commit can do: qnn_conv2d_forward on the block-diagonal (3, 3, C, C) kernel with the same
             epilogue, on whatever route the dispatcher picks (the kernel name is recorded).

Both produce the same packed words (checked before timing).  Device events around `--iters` back-to-back calls, the two
forms alternated `--rounds` times after a warm-up; prints one JSON line per (map, C) with the median time per call, the
lowest and highest round, the bytes `depthwise` moves (input and output tensors as stored, the weight table once) and the
fraction of the 8 TB/s HBM figure those bytes over that time are.

    python tools/bench_depthwise.py [--iters 20] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qnn_amd                                   # noqa: E402,F401
from qnn_amd import _abi                         # noqa: E402

HBM = 8.0e12
MAPS = ((4096, 16, 16), (64, 112, 112))
CHANNELS = (32, 64, 128, 256)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depthwise.py needs a GPU")
    store, bits = _abi.STORE_I4, 4
    for N, H, W in MAPS:
        for C in CHANNELS:
            g = torch.Generator(device="cuda").manual_seed(1)
            x = torch.randint(-8, 8, (N * H * W, C), device="cuda", generator=g).float() / 8
            xp = _abi.pack(x, C, _abi.FN_GRID, bits, store)
            del x
            k = torch.randint(-8, 8, (3, 3, C, 1), device="cuda", generator=g).float() / 8
            full = torch.zeros((3, 3, C, C), device="cuda")
            idx = torch.arange(C, device="cuda")
            full[:, :, idx, idx] = k[:, :, :, 0]
            inv = torch.rand(C, device="cuda", generator=g) * 0.5 + 0.25
            shift = torch.rand(C, device="cuda", generator=g) - 0.5
            wd = _abi.DepthwiseWeights(_abi.W_QUANT, 4, 1.0, k, None, 1, True, store)
            wf = _abi.Weights(_abi.W_QUANT, 4, 1.0, full, None, 1, True, store)
            words = _abi.words(store, C)
            yd = torch.empty((N * H * W, words), dtype=torch.int32, device="cuda")
            yf = torch.empty_like(yd)

            def depthwise():
                return _abi.depthwise(wd, xp, store, bits, N, H, W, inv, shift, _abi.FN_QUANTIZED_TANH, 4, store, out=yd)[0]

            def expanded():
                return _abi.conv2d(wf, xp, store, bits, N, H, W, inv, shift, _abi.FN_QUANTIZED_TANH, 4, 1, store, out=yf)[0]

            depthwise()
            kd = _abi.last_kernel()
            expanded()
            kf = _abi.last_kernel()
            assert torch.equal(yd, yf), "the two forms disagree"
            for fn in (depthwise, expanded):                    # warm-up
                timed(fn, 3)
            td, tf = [], []
            for _ in range(args.rounds):
                td.append(timed(depthwise, args.iters))
                tf.append(timed(expanded, args.iters))
            nbytes = xp.numel() * 4 + yd.numel() * 4 + 9 * words * 4 * 4
            d, f = statistics.median(td), statistics.median(tf)
            us = lambda t: round(t * 1e6, 1)                    # noqa: E731
            print(json.dumps({"store": "i4", "map": [N, H, W, C], "depthwise_kernel": kd, "expanded_kernel": kf,
                              "depthwise_us": us(d), "depthwise_us_min_max": [us(min(td)), us(max(td))],
                              "expanded_us": us(f), "expanded_us_min_max": [us(min(tf)), us(max(tf))],
                              "depthwise_bytes": nbytes, "depthwise_hbm_fraction": round(nbytes / d / HBM, 3),
                              "speedup": round(f / d, 2),
                              "faster_beyond_bracket": bool(max(td) < min(tf))}), flush=True)
            del xp, full, wd, wf, yd, yf


if __name__ == "__main__":
    main()
