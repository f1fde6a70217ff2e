"""Time the channel concatenation of packed activations two ways (profiles/concat/README.md):

  route   what a concat of packed tensors costs without qnn_concat_forward: unpack every input to float32 -> torch.cat ->
          pack for the next layer, the pieces timed together;
  codes   qnn_concat_forward on the packed words (concat_i4 / concat_bin).

Both produce the same packed words (checked).  Device events around `--iters` back-to-back calls, the two forms
alternated `--rounds` times after a warm-up; prints one JSON line per (store, channel list) with the median time per call,
every round's time (the spread), the bytes each form moves (tensors as stored) and the fraction of the 8 TB/s HBM figure
those bytes over that time are.

    python tools/bench_concat.py [--pixels 4096 32 32] [--iters 20] [--rounds 5]
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
LISTS = ([64, 64], [12, 24, 36])


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
    ap.add_argument("--pixels", type=int, nargs=3, default=[4096, 32, 32])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_concat.py needs a GPU")
    N, H, W = args.pixels
    P = N * H * W
    for name, store, bits in (("i4", _abi.STORE_I4, 4), ("bin", _abi.STORE_BIN, 1)):
        for channels in LISTS:
            g = torch.Generator(device="cuda").manual_seed(1)
            m = 2 ** (bits - 1)
            xs = []
            for c in channels:
                x = (torch.randint(-m, m, (P, c), device="cuda", generator=g).float() / m) if bits > 1 else \
                    (torch.randint(0, 2, (P, c), device="cuda", generator=g).float() * 2 - 1)
                xs.append(_abi.pack(x, c, _abi.FN_GRID, bits, store))
                del x
            total = sum(channels)

            def route():
                fs = [_abi.unpack(p, P, c, store, bits) for p, c in zip(xs, channels)]
                return _abi.pack(torch.cat(fs, dim=-1), total, _abi.FN_GRID, bits, store)

            def codes():
                return _abi.concat(xs, channels, store, bits, P)

            ya, yb = route(), codes()
            kernel = _abi.last_kernel()
            assert torch.equal(ya, yb), "the two forms disagree"
            del ya, yb
            for fn in (route, codes):                    # warm-up
                timed(fn, 3)
            tr, tc = [], []
            for _ in range(args.rounds):
                tr.append(timed(route, args.iters))
                tc.append(timed(codes, args.iters))
            pin = sum(p.numel() for p in xs) * 4
            pout = P * _abi.words(store, total) * 4
            f = P * total * 4
            b_route = (pin + f) + (f + f) + (f + pout)   # unpack, cat, pack: each reads and writes once
            b_codes = pin + pout
            r, c = statistics.median(tr), statistics.median(tc)
            print(json.dumps({"store": name, "pixels": [N, H, W], "channels": channels, "kernel": kernel,
                              "route_us": round(r * 1e6, 1), "route_us_all": [round(t * 1e6, 1) for t in tr],
                              "codes_us": round(c * 1e6, 1), "codes_us_all": [round(t * 1e6, 1) for t in tc],
                              "route_bytes": b_route, "codes_bytes": b_codes,
                              "route_hbm_fraction": round(b_route / r / HBM, 3),
                              "codes_hbm_fraction": round(b_codes / c / HBM, 3), "speedup": round(r / c, 2)}), flush=True)
            del xs


if __name__ == "__main__":
    main()
