#!/usr/bin/env python3
"""The un-folded int4 strip kernels with each quantised activation, for a run under `rocprofv3 --kernel-trace --stats`
(the kernel names carry the template arguments: the last one is the activation, 0 = quantized_tanh, 6 = quantized_relu,
7 = quantized_leakyrelu).  Shapes of DESIGN.md 3.2: 64 x 224^2 x 16, 64 x 112^2 x 32, 64 x 56^2 x 64 without and with the
packed shortcut merge.  The activations alternate launch by launch.
Usage: tools/bench_qrelu.py [reps] [fn,fn,...]     fn: quantized_tanh | quantized_relu | quantized_leakyrelu
(a tree without the two new functions runs `quantized_tanh` alone: the yardstick from the parent commit)."""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
pkg = importlib.import_module("quantizedneuralnetworks-keras-tensorflow_amd")
_abi, engine = pkg._abi, pkg.engine
F32 = np.float32
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
names = sys.argv[2].split(",") if len(sys.argv) > 2 else ["quantized_tanh", "quantized_relu", "quantized_leakyrelu"]
FN = {n: getattr(_abi, "FN_" + n.upper()) for n in names}
rng = np.random.default_rng(0)
rows = []
for n, hw, c, res in ((64, 224, 16, False), (64, 112, 32, False), (64, 56, 64, False), (64, 56, 64, True)):
    op = {"op": "conv", "kind": "quantized", "nb": 4, "kernel": rng.uniform(-1, 1, (3, 3, c, c)).astype(F32), "bias": None,
          "strides": (1, 1), "padding": "same"}
    var = 9 * c * 0.12
    bn = dict(op="bn", eps=1e-3, gamma=rng.uniform(0.5, 1.5, c).astype(F32), beta=(rng.standard_normal(c) * 0.5).astype(F32),
              mean=(rng.standard_normal(c) * 0.1 * np.sqrt(var)).astype(F32), var=(var * rng.uniform(0.8, 1.25, c)).astype(F32))
    w = engine._prepack(op, _abi.STORE_I4, torch.device("cuda"), stride=1, same_pad=True)
    i, s = engine.bn_constants(bn)
    inv, shift = torch.as_tensor(i).cuda(), torch.as_tensor(s).cuda()
    x = torch.randint(-2**31, 2**31 - 1, (n * hw * hw, c // 8), dtype=torch.int32, device="cuda")
    sc = torch.randint(-2**31, 2**31 - 1, (n * hw * hw, c // 8), dtype=torch.int32, device="cuda")
    y = torch.empty_like(x)
    kw = dict(res=sc, res_store=_abi.STORE_I4, res_bits=4, post_scale=0.5) if res else {}
    row = {"shape": "%dx%d^2x%d%s" % (n, hw, c, "+merge" if res else "")}
    for _ in range(reps):
        for name in names:                      # alternating; no fold is passed: the un-folded chain
            _abi.conv2d(w, x, _abi.STORE_I4, 4, n, hw, hw, inv, shift, FN[name], 4, 1, _abi.STORE_I4, out=y, **kw)
            row[name] = _abi.last_kernel()
    torch.cuda.synchronize()
    rows.append(row)
print(json.dumps(rows))
