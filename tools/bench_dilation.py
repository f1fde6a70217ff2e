#!/usr/bin/env python3
"""One dilated 3x3 'same' int4 -> int4 layer alone, launched `reps` times back to back: meant to be run under
rocprofv3 in a run of its own, which gives the time per launch of the kernel it names:

    rocprofv3 --kernel-trace --stats -d out -- python tools/bench_dilation.py 64 56 64 --dil 2 --merge
    rocprofv3 --kernel-trace --stats -d out -- python tools/bench_dilation.py 64 56 64 --dil 2 --merge --no-strip

Arguments: N, H (= W), C (Cin = Cout: 16 / 32 / 64).  --dil 1 is the undilated layer (strip_i4_c<cin>, unfolded: the
yardstick of the same MACs and bytes; run it on the parent commit as well).  --merge adds the packed int4 shortcut with
post_scale 0.5; --no-strip passes QNN_EPI_NO_STRIP (k_conv_generic for a dilated layer).  Prints one JSON line: kernel
name, HIP-event time per launch (a cross-check of the trace, same run), a digest of the output.  Without rocprofv3 it is
an ordinary timing run.  bench.py is not involved."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import torch                # noqa: E402

pkg = importlib.import_module("quantizedneuralnetworks-keras-tensorflow_amd")
_abi, engine = pkg._abi, pkg.engine
F32 = np.float32

ap = argparse.ArgumentParser()
ap.add_argument("n", type=int)
ap.add_argument("hw", type=int)
ap.add_argument("c", type=int)
ap.add_argument("--dil", type=int, default=2)
ap.add_argument("--merge", action="store_true")
ap.add_argument("--no-strip", action="store_true")
ap.add_argument("--reps", type=int, default=100)
a = ap.parse_args()

rng = np.random.default_rng(0)
torch.manual_seed(0)           # the same codes in every process: digests of two runs of one shape are comparable
n, hw, c = a.n, a.hw, a.c
op = {"op": "conv", "kind": "quantized", "nb": 4, "kernel": rng.uniform(-1, 1, (3, 3, c, c)).astype(F32), "bias": None,
      "strides": (1, 1), "padding": "same", "dilation_rate": (a.dil, a.dil)}
var = 9 * c * 0.12
bn = dict(op="bn", eps=1e-3, gamma=rng.uniform(0.5, 1.5, c).astype(F32), beta=(rng.standard_normal(c) * 0.5).astype(F32),
          mean=(rng.standard_normal(c) * 0.1 * np.sqrt(var)).astype(F32), var=(var * rng.uniform(0.8, 1.25, c)).astype(F32))
w = engine._prepack(op, _abi.STORE_I4, torch.device("cuda"), stride=1, same_pad=True)
i, s = engine.bn_constants(bn)
inv, shift = torch.as_tensor(i).cuda(), torch.as_tensor(s).cuda()
x = torch.randint(-2**31, 2**31 - 1, (n * hw * hw, c // 8), dtype=torch.int32, device="cuda")
sc = torch.randint(-2**31, 2**31 - 1, (n * hw * hw, c // 8), dtype=torch.int32, device="cuda")
y = torch.empty_like(x)
kw = dict(res=sc, res_store=_abi.STORE_I4, res_bits=4, post_scale=0.5) if a.merge else {}
if a.no_strip:
    _abi.set_option("strip", 0)


def launch():
    _abi.conv2d(w, x, _abi.STORE_I4, 4, n, hw, hw, inv, shift, _abi.FN_QUANTIZED_TANH, 4, 1, _abi.STORE_I4, out=y, **kw)


for _ in range(10):
    launch()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(a.reps):
    launch()
e1.record()
torch.cuda.synchronize()
print(json.dumps({"kernel": _abi.last_kernel(), "n": n, "hw": hw, "c": c, "dil": a.dil, "merge": a.merge,
                  "us_per_launch_events": round(e0.elapsed_time(e1) * 1e3 / a.reps, 2),
                  "digest": int(y.to(torch.int64).sum().item())}))
