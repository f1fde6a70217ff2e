"""Time a stride-2 'same' transposed convolution on int4 codes (4-bit weights, BN + quantized_tanh(4) to int4) three ways
(profiles/tconv/README.md):

  mfma    qnn_tconv_forward on the matrix-pipe form (tconv_i4_mfma);
  plain   qnn_tconv_forward on the plain form (tconv_i4_plain), forced two ways, both timed: `plain_v1` writes the same
          int4 words through an output pointer 4 bytes off its 16-byte alignment (one word per lane), `plain_i8` keeps
          the alignment (four words per lane) and writes the same codes to the int8 store (twice the output bytes);
  conv1x1 for the 2x2 window only: qnn_conv2d_forward on the (1, 1, Cin, 4 * Cout) kernel that computes the same sums
          before the depth-to-space shuffle -- the closest thing the library can run without this entry.  It skips the
          shuffle, so it is a lower bound on that route's cost.

mfma, plain_v1 and (shuffled) conv1x1 produce the same packed words; plain_i8 the same codes (checked before timing).
Device events around `--iters` back-to-back calls, the forms alternated `--rounds` times after a warm-up; prints one JSON
line per (window, map, C) with the median time per call, the lowest and highest round, the bytes mfma moves (input and
output tensors as stored, the operand image once) and the fraction of the 8 TB/s HBM figure those bytes over that time are.

    python tools/bench_tconv.py [--iters 20] [--rounds 5]
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
MAPS = ((4096, 8, 8), (64, 56, 56))
CHANNELS = (64, 128, 256)
WINDOWS = (2, 4)


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
    ap.add_argument("--channels", type=int, nargs="*", default=list(CHANNELS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tconv.py needs a GPU")
    I4, I8, bits = _abi.STORE_I4, _abi.STORE_I8, 4
    QT = _abi.FN_QUANTIZED_TANH
    for k in WINDOWS:
        for N, H, W in MAPS:
            for C in args.channels:
                g = torch.Generator(device="cuda").manual_seed(1)
                x = torch.randint(-8, 8, (N * H * W, C), device="cuda", generator=g).float() / 8
                xp = _abi.pack(x, C, _abi.FN_GRID, bits, I4)
                del x
                kern = torch.randint(-8, 8, (k, k, C, C), device="cuda", generator=g).float() / 8      # (kh, kw, Cout, Cin)
                inv = (torch.rand(C, device="cuda", generator=g) * 0.5 + 0.25) / (C ** 0.5)
                shift = torch.rand(C, device="cuda", generator=g) - 0.5
                wt = _abi.TConvWeights(_abi.W_QUANT, 4, 1.0, kern, None, 2, True, I4)
                Ho, Wo = wt.out_hw(H, W)
                pix = N * Ho * Wo
                cw = _abi.words(I4, C)
                ym = torch.empty((pix, cw), dtype=torch.int32, device="cuda")
                buf = torch.empty(pix * cw + 4, dtype=torch.int32, device="cuda")
                yv = buf[1:1 + pix * cw].view(pix, cw)
                y8 = torch.empty((pix, _abi.words(I8, C)), dtype=torch.int32, device="cuda")
                forms = {
                    "mfma": lambda: _abi.tconv(wt, xp, I4, bits, N, H, W, inv, shift, QT, 4, I4, out=ym),
                    "plain_v1": lambda: _abi.tconv(wt, xp, I4, bits, N, H, W, inv, shift, QT, 4, I4, out=yv),
                    "plain_i8": lambda: _abi.tconv(wt, xp, I4, bits, N, H, W, inv, shift, QT, 4, I8, out=y8),
                }
                if k == 2:
                    # w1[0, 0, c, (ky * 2 + kx) * Cout + f] = kern[ky, kx, f, c]
                    w1 = kern.permute(3, 0, 1, 2).reshape(1, 1, C, 4 * C).contiguous()
                    wc = _abi.Weights(_abi.W_QUANT, 4, 1.0, w1, None, 1, True, I4)
                    inv4, shift4 = inv.repeat(4).contiguous(), shift.repeat(4).contiguous()
                    yc = torch.empty((N * H * W, 4 * cw), dtype=torch.int32, device="cuda")
                    forms["conv1x1"] = lambda: _abi.conv2d(wc, xp, I4, bits, N, H, W, inv4, shift4, QT, 4, 1, I4, out=yc)
                names = {}
                for name, fn in forms.items():
                    fn()
                    names[name] = _abi.last_kernel()
                assert names["mfma"] == "tconv_i4_mfma" and names["plain_v1"] == names["plain_i8"] == "tconv_i4_plain", names
                assert torch.equal(ym, yv), "the matrix-pipe and the plain form disagree"
                codes = lambda t, store: _abi.unpack(t, pix, C, store, 4)              # noqa: E731
                assert torch.equal(codes(ym, I4), codes(y8, I8)), "the int8-store plain form disagrees"
                if k == 2:
                    shuffled = yc.view(N, H, W, 2, 2, cw).permute(0, 1, 3, 2, 4, 5).reshape(pix, cw)
                    assert torch.equal(ym, shuffled), "the 1x1 convolution disagrees"
                    del shuffled
                for fn in forms.values():                               # warm-up
                    timed(fn, 3)
                t = {name: [] for name in forms}
                for _ in range(args.rounds):
                    for name, fn in forms.items():
                        t[name].append(timed(fn, args.iters))
                us = lambda v: round(v * 1e6, 1)                        # noqa: E731
                med = {name: statistics.median(v) for name, v in t.items()}
                nbytes = xp.numel() * 4 + ym.numel() * 4 + k * k * C * C
                plain = min(("plain_v1", "plain_i8"), key=lambda n: med[n])
                row = {"store": "i4", "window": k, "map": [N, H, W, C], "kernels": names,
                       "mfma_bytes": nbytes, "mfma_hbm_fraction": round(nbytes / med["mfma"] / HBM, 3),
                       "faster_plain": plain, "speedup_over_plain": round(med[plain] / med["mfma"], 2),
                       "faster_beyond_bracket": bool(max(t["mfma"]) < min(t[plain]))}
                for name in forms:
                    row[name + "_us"] = us(med[name])
                    row[name + "_us_min_max"] = [us(min(t[name])), us(max(t[name]))]
                if k == 2:
                    row["ratio_to_conv1x1"] = round(med["mfma"] / med["conv1x1"], 2)
                print(json.dumps(row), flush=True)
                del xp, kern, wt, ym, buf, yv, y8, forms


if __name__ == "__main__":
    main()
