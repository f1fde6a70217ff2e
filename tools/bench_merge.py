"""Time every kernel family of qnn_merge_forward against what the engine would do without it, on the same tensors in the
same process (profiles/merge/README.md):

  float32             merge_f32 against the torch op (a + b, torch.maximum);
  codes -> codes      merge_bin / _i4 / _i8 / _t2 against qnn_unpack_f32 of both inputs -> torch op -> qnn_pack_f32;
  codes -> float32    merge_*_f32 against qnn_unpack_f32 of both inputs -> torch op.

Both forms produce the same tensor (checked).  Device events around `--iters` back-to-back calls (`--base-iters` of the
baseline), the two forms alternated `--rounds` times after a warm-up, and the baseline once more at the end, so its own
spread over the run is on record.  One JSON line per (family, op): the median time per call, every round's time, the bytes
each form moves (tensors as stored, each read or written once per kernel) and the fraction of the 8 TB/s HBM figure those
bytes over that time are.

    python tools/bench_merge.py [--pixels 4096 32 32] [--channels 64] [--iters 20] [--base-iters 5] [--rounds 5]
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
TORCH = {"add": torch.add, "sub": torch.sub, "mul": torch.mul, "max": torch.maximum, "min": torch.minimum}
CASES = [("f32", "add"), ("f32", "max"), ("bin", "max"), ("bin", "mul"), ("i4", "max"), ("i8", "max"), ("t2", "max"), ("t2", "mul"),
         ("bin", "add"), ("i4", "add"), ("i4", "mul"), ("i8", "add"), ("t2", "add")]
STORE = {"f32": (_abi.STORE_F32, 0), "bin": (_abi.STORE_BIN, 1), "i4": (_abi.STORE_I4, 4), "i8": (_abi.STORE_I8, 8),
         "t2": (_abi.STORE_T2, 1)}


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
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--base-iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_merge.py needs a GPU")
    N, H, W = args.pixels
    P, C = N * H * W, args.channels
    g = torch.Generator(device="cuda").manual_seed(1)
    for kind, op in CASES:
        store, bits = STORE[kind]
        xs = []
        for _ in range(2):
            if kind == "f32":
                xs.append(torch.randn((P, C), device="cuda", generator=g))
                continue
            m = 2 ** (bits - 1)
            x = (torch.randint(0, 2, (P, C), device="cuda", generator=g).float() * 2 - 1) if kind == "bin" else \
                torch.randint(-1, 2, (P, C), device="cuda", generator=g).float() if kind == "t2" else \
                torch.randint(-m, m, (P, C), device="cuda", generator=g).float() / m
            xs.append(_abi.pack(x, C, _abi.FN_GRID, bits, store))
            del x
        out_store = _abi.merge_out_store(op, store)

        def base():
            if kind == "f32":
                return TORCH[op](xs[0], xs[1])
            y = TORCH[op](_abi.unpack(xs[0], P, C, store, bits), _abi.unpack(xs[1], P, C, store, bits))
            return y if out_store == _abi.STORE_F32 else _abi.pack(y, C, _abi.FN_GRID, bits, store)

        def kern():
            return _abi.merge(xs, op, store, bits, P, C)[0]

        ya, yb = base(), kern()
        kernel = _abi.last_kernel()
        assert torch.equal(ya, yb), "the two forms disagree: %s %s" % (kind, op)
        del ya, yb
        for fn in (base, kern):                      # warm-up
            timed(fn, 3)
        tb, tk = [], []
        for _ in range(args.rounds):
            tb.append(timed(base, args.base_iters))
            tk.append(timed(kern, args.iters))
        tb.append(timed(base, args.base_iters))      # the baseline again, behind the last kernel round
        f = P * C * 4
        pin = sum(x.numel() for x in xs) * 4
        pout = f if out_store == _abi.STORE_F32 else xs[0].numel() * 4
        if kind == "f32":
            b_base = pin + pout
        else:                                        # two unpacks, the torch op, the pack (codes out only)
            b_base = (pin + 2 * f) + 3 * f + ((f + pout) if out_store != _abi.STORE_F32 else 0)
        b_kern = pin + pout
        b, k = statistics.median(tb), statistics.median(tk)
        print(json.dumps({"store": kind, "op": op, "pixels": [N, H, W], "channels": C, "n": 2, "kernel": kernel,
                          "base_us": round(b * 1e6, 1), "base_us_all": [round(t * 1e6, 1) for t in tb],
                          "kernel_us": round(k * 1e6, 1), "kernel_us_all": [round(t * 1e6, 1) for t in tk],
                          "base_bytes": b_base, "kernel_bytes": b_kern,
                          "base_hbm_fraction": round(b_base / b / HBM, 3),
                          "kernel_hbm_fraction": round(b_kern / k / HBM, 3), "speedup": round(b / k, 2)}), flush=True)
        del xs


if __name__ == "__main__":
    main()
