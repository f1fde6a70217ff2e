"""Time a zero pad and a nearest-neighbour repeat of a packed int4 activation two ways (profiles/spatial/README.md):

  route   what the op costs behind a packed activation without qnn_spatial2d_forward: unpack to float32 -> torch (pad /
          repeat_interleave) -> pack for the next layer, the pieces timed together;
  codes   qnn_spatial2d_forward on the packed words (spatial_i4).

Both produce the same packed words (checked).  Device events around `--iters` back-to-back calls, the two forms
alternated `--rounds` times after a warm-up; prints one JSON line per (map, op) with the median time per call, every
round's time (the spread), the bytes each form moves (tensors as stored) and the fraction of the 8 TB/s HBM figure those
bytes over that time are.

    python tools/bench_spatial.py [--iters 20] [--rounds 5]
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
MAPS = ((4096, 16, 16, 64), (64, 224, 224, 64))
OPS = (("pad1", dict(pad=1)), ("up2", dict(up=(2, 2))))


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
        raise SystemExit("bench_spatial.py needs a GPU")
    store, bits = _abi.STORE_I4, 4
    for N, H, W, C in MAPS:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randint(-8, 8, (N * H * W, C), device="cuda", generator=g).float() / 8
        xp = _abi.pack(x, C, _abi.FN_GRID, bits, store)
        del x
        for name, kw in OPS:
            Ho, Wo = _abi.spatial2d_out_hw(H, W, **kw)

            def route():
                f = _abi.unpack(xp, N * H * W, C, store, bits).reshape(N, H, W, C)
                if "pad" in kw:
                    f = torch.nn.functional.pad(f, (0, 0, 1, 1, 1, 1))
                else:
                    f = f.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
                return _abi.pack(f, C, _abi.FN_GRID, bits, store)

            def codes():
                return _abi.spatial2d(xp, store, bits, N, H, W, C, **kw)[0]

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
            pin, pout = xp.numel() * 4, N * Ho * Wo * _abi.words(store, C) * 4
            fin, fout = N * H * W * C * 4, N * Ho * Wo * C * 4
            # unpack, the torch op (the repeat: two passes, rows then columns), pack: each reads and writes once
            mid = (fin + fout) if "pad" in kw else (fin + N * 2 * H * W * C * 4) + (N * 2 * H * W * C * 4 + fout)
            b_route = (pin + fin) + mid + (fout + pout)
            b_codes = pin + pout
            r, c = statistics.median(tr), statistics.median(tc)
            print(json.dumps({"store": "i4", "map": [N, H, W, C], "op": name, "kernel": kernel,
                              "route_us": round(r * 1e6, 1), "route_us_all": [round(t * 1e6, 1) for t in tr],
                              "codes_us": round(c * 1e6, 1), "codes_us_all": [round(t * 1e6, 1) for t in tc],
                              "route_bytes": b_route, "codes_bytes": b_codes,
                              "route_hbm_fraction": round(b_route / r / HBM, 3),
                              "codes_hbm_fraction": round(b_codes / c / HBM, 3), "speedup": round(r / c, 2)}), flush=True)
        del xp


if __name__ == "__main__":
    main()
