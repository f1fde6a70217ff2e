#!/usr/bin/env python3
"""Hidden dense layers through qnn_dense_forward (csrc/qnn_dense_mfma.hip and what ran them before), one process per
checkout: I4 / I8 / BIN operands on 64 x 1024 -> 1024, 256 x 2048 -> 2048, 4096 x 1024 -> 1024 and 4096 x 8192 -> 1024, each
with float32 output (no activation) and with packed output (I4 and I8: quantized_tanh into the operands' store; BIN:
binary_tanh into I4 codes), bias and BN on.

Per case: one warm-up launch, one timed launch to size the window, then `reps` windows of back-to-back launches between
two HIP events (about 20 ms of work each, 1 to 500 launches); microseconds per launch as median / min / max over the
windows, the kernel qnn_last_kernel names, and a checksum of the output (the sum of its words) to compare two checkouts.
Usage: tools/bench_dense.py [reps] [ROOT]      ROOT: the checkout to import the package from (default: this one); runs
of two checkouts are alternated process by process (profiles/dense_mfma/README.md).  Prints one JSON line."""
import importlib, json, os, sys
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
ROOT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
pkg = importlib.import_module("quantizedneuralnetworks-keras-tensorflow_amd")
_abi, engine = pkg._abi, pkg.engine
F32 = np.float32
SHAPES = [(64, 1024, 1024), (256, 2048, 2048), (4096, 1024, 1024), (4096, 8192, 1024)]
# operand store: (name, bits, weight kind, packed output: store, fn, act_bits)
STORES = {_abi.STORE_I4: ("i4", 4, "quantized", _abi.STORE_I4, _abi.FN_QUANTIZED_TANH, 4),
          _abi.STORE_I8: ("i8", 8, "quantized", _abi.STORE_I8, _abi.FN_QUANTIZED_TANH, 8),
          _abi.STORE_BIN: ("bin", 1, "binary", _abi.STORE_I4, _abi.FN_BINARY_TANH, 0)}


def window(call, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def timed(call):
    call()
    n = int(min(500, max(1, 20000.0 / max(window(call, 1), 1.0))))
    t = sorted(window(call, n) for _ in range(reps))
    return {"us_median": round(t[len(t) // 2], 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2), "launches": n}


rows = {}
for N, K, U in SHAPES:
    for store, (name, bits, kind, pstore, pfn, pbits) in STORES.items():
        rng = np.random.default_rng(K + U + store)
        op = {"op": "dense", "kind": kind, "nb": bits, "kernel": rng.uniform(-1, 1, (K, U)).astype(F32),
              "bias": (rng.standard_normal(U) * 0.05).astype(F32)}
        w = engine._prepack(op, store, "cuda")
        inv = torch.as_tensor((rng.uniform(0.5, 1.5, U) * rng.choice([-1.0, 1.0], U) / np.sqrt(K)).astype(F32)).cuda()
        shift = torch.as_tensor((rng.standard_normal(U) * 0.1).astype(F32)).cuda()
        m = 2 ** (bits - 1)
        x = (rng.integers(0, 2, (N, K)) * 2 - 1 if bits == 1 else rng.integers(-m, m, (N, K)) / m).astype(F32)
        xp = _abi.pack(torch.as_tensor(x).cuda(), K, _abi.FN_BINARY_TANH if bits == 1 else _abi.FN_GRID, bits, store)
        for out_name, out_store, fn, ab in (("f32", _abi.STORE_F32, _abi.FN_NONE, 0), ("packed", pstore, pfn, pbits)):
            y = _abi.dense(w, xp, store, bits, N, inv, shift, fn, ab, out_store)
            r = timed(lambda: _abi.dense(w, xp, store, bits, N, inv, shift, fn, ab, out_store, out=y))
            r["kernel"] = _abi.last_kernel()
            r["checksum"] = int(y.view(torch.int32).to(torch.int64).sum().item())
            rows["%dx%d->%d %s->%s" % (N, K, U, name, out_name)] = r
print(json.dumps({"root": ROOT, "reps": reps, "cases": rows}))
