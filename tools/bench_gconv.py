"""Time a 3x3 'same' stride-1 grouped layer on int4 codes (4-bit weights, BN + quantized_tanh(4) to int4) three ways
(profiles/gconv/README.md):

  mfma      qnn_gconv_forward on 16-byte aligned tensors (gconv_i4_mfma, the matrix-pipe form);
  plain     the same call through a view 4 bytes off the alignment (gconv_i4_plain, the gather);
  expanded  what the parent commit can do: qnn_conv2d_forward on the block-diagonal (3, 3, Cin, Cout) kernel with the same
            epilogue, on whatever route the dispatcher picks (the kernel name is recorded).

All three produce the same packed words (checked before timing).  Device events around `--iters` back-to-back calls, the
forms alternated `--rounds` times after a warm-up; prints one JSON line per shape with the median time per call and the
lowest and highest round of each form.

    python tools/bench_gconv.py [--iters 20] [--rounds 5]
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

SHAPES = ((64, 56, 56, 128, 32), (64, 28, 28, 256, 32), (64, 14, 14, 512, 32), (64, 7, 7, 1024, 32),
          (4096, 16, 16, 128, 2), (4096, 16, 16, 128, 8), (4096, 16, 16, 128, 32))      # N, H, W, C, groups


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def off_view(t):
    """A contiguous copy of `t` that starts 4 bytes behind a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gconv.py needs a GPU")
    store, bits = _abi.STORE_I4, 4
    for N, H, W, C, G in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randint(-8, 8, (N * H * W, C), device="cuda", generator=g).float() / 8
        xp = _abi.pack(x, C, _abi.FN_GRID, bits, store)
        del x
        cg = C // G
        k = torch.randint(-8, 8, (3, 3, cg, C), device="cuda", generator=g).float() / 8
        full = torch.zeros((3, 3, C, C), device="cuda")
        for grp in range(G):
            full[:, :, grp * cg:(grp + 1) * cg, grp * cg:(grp + 1) * cg] = k[:, :, :, grp * cg:(grp + 1) * cg]
        inv = torch.rand(C, device="cuda", generator=g) * 0.25 + 0.125
        shift = torch.rand(C, device="cuda", generator=g) - 0.5
        wg = _abi.GConvWeights(_abi.W_QUANT, 4, 1.0, k, None, G, 1, True, store)
        wf = _abi.Weights(_abi.W_QUANT, 4, 1.0, full, None, 1, True, store)
        words = _abi.words(store, C)
        ym = torch.empty((N * H * W, words), dtype=torch.int32, device="cuda")
        yf = torch.empty_like(ym)
        xo, yo = off_view(xp), off_view(ym)

        def mfma():
            return _abi.gconv(wg, xp, store, bits, N, H, W, inv, shift, _abi.FN_QUANTIZED_TANH, 4, store, out=ym)[0]

        def plain():
            return _abi.gconv(wg, xo, store, bits, N, H, W, inv, shift, _abi.FN_QUANTIZED_TANH, 4, store, out=yo)[0]

        def expanded():
            return _abi.conv2d(wf, xp, store, bits, N, H, W, inv, shift, _abi.FN_QUANTIZED_TANH, 4, 1, store, out=yf)[0]

        forms = (mfma, plain, expanded)
        names = []
        for fn in forms:
            fn()
            names.append(_abi.last_kernel())
        assert names[0] == "gconv_i4_mfma" and names[1] == "gconv_i4_plain", names
        assert torch.equal(ym, yo) and torch.equal(ym, yf), "the forms disagree"
        for fn in forms:                                        # warm-up
            timed(fn, 3)
        t = [[], [], []]
        for _ in range(args.rounds):
            for i, fn in enumerate(forms):
                t[i].append(timed(fn, args.iters))
        med = [statistics.median(v) for v in t]
        us = lambda v: round(v * 1e6, 1)                        # noqa: E731
        print(json.dumps({"store": "i4", "map": [N, H, W, C], "groups": G, "expanded_kernel": names[2],
                          "mfma_us": us(med[0]), "mfma_us_min_max": [us(min(t[0])), us(max(t[0]))],
                          "plain_us": us(med[1]), "plain_us_min_max": [us(min(t[1])), us(max(t[1]))],
                          "expanded_us": us(med[2]), "expanded_us_min_max": [us(min(t[2])), us(max(t[2]))],
                          "mfma_over_plain": round(med[1] / med[0], 2), "mfma_over_expanded": round(med[2] / med[0], 2),
                          "mfma_beats_plain_beyond_bracket": bool(max(t[0]) < min(t[1])),
                          "mfma_beats_expanded_beyond_bracket": bool(max(t[0]) < min(t[2]))}), flush=True)
        del xp, xo, full, wg, wf, ym, yo, yf


if __name__ == "__main__":
    main()
