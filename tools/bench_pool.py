"""Time a stand-alone 2x2 / 2 max-pool of a packed activation two ways (profiles/pool/README.md):

  route   what the engines did before qnn_pool2d_forward: unpack to float32 -> torch max-pool (engine._maxpool) ->
          pack for the next layer, the three pieces timed together;
  codes   qnn_pool2d_forward on the packed words (pool_max_i4 / pool_max_bin).

Both produce the same packed words (checked).  Device events around `--iters` back-to-back calls, the two forms
alternated `--rounds` times; prints one JSON line per store with the median time per call, the bytes each form moves
(tensors as stored) and the fraction of the 8 TB/s HBM figure those bytes over that time are.

    python tools/bench_pool.py [--shape 4096 32 32 64] [--iters 20] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qnn_amd                                   # noqa: E402,F401
from qnn_amd import _abi, engine                 # noqa: E402

HBM = 8.0e12


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
    ap.add_argument("--shape", type=int, nargs=4, default=[4096, 32, 32, 64])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pool.py needs a GPU")
    N, H, W, C = args.shape
    op = {"op": "maxpool", "size": 2}
    for name, store, bits in (("i4", _abi.STORE_I4, 4), ("bin", _abi.STORE_BIN, 1)):
        g = torch.Generator(device="cuda").manual_seed(1)
        m = 2 ** (bits - 1)
        x = (torch.randint(-m, m, (N, H, W, C), device="cuda", generator=g).float() / m) if bits > 1 else \
            (torch.randint(0, 2, (N, H, W, C), device="cuda", generator=g).float() * 2 - 1)
        xp = _abi.pack(x, C, _abi.FN_GRID, bits, store)
        del x
        cw = xp.shape[1]

        def route():
            f = _abi.unpack(xp, N * H * W, C, store, bits).reshape(N, H, W, C)
            p = engine._maxpool(f, op)
            return _abi.pack(p.contiguous(), C, _abi.FN_GRID, bits, store)

        def codes():
            return _abi.pool2d(xp, store, bits, N, H, W, C, _abi.POOL_MAX, 2)[0]

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
        pin, pout = N * H * W * cw * 4, N * (H // 2) * (W // 2) * cw * 4
        fin, fout = N * H * W * C * 4, N * (H // 2) * (W // 2) * C * 4
        b_route = (pin + fin) + (fin + fout) + (fout + pout)        # unpack, max-pool, pack: each reads and writes once
        b_codes = pin + pout
        r, c = statistics.median(tr), statistics.median(tc)
        print(json.dumps({"store": name, "shape": [N, H, W, C], "kernel": kernel,
                          "route_us": round(r * 1e6, 1), "route_us_all": [round(t * 1e6, 1) for t in tr],
                          "codes_us": round(c * 1e6, 1), "codes_us_all": [round(t * 1e6, 1) for t in tc],
                          "route_bytes": b_route, "codes_bytes": b_codes,
                          "route_hbm_fraction": round(b_route / r / HBM, 3), "codes_hbm_fraction": round(b_codes / c / HBM, 3),
                          "speedup": round(r / c, 2)}), flush=True)


if __name__ == "__main__":
    main()
