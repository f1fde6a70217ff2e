#!/usr/bin/env python3
"""Float32-activation convolutions (csrc/qnn_f32act.hip) against k_conv_generic (qnn_set_conv_impl(1)).

    python tools/bench_f32act.py [--n 4096] [--reps 20] [--out profiles/f32act/bench.json]

Per layer (the CIFAR ResNet-20 shapes, the two 1x1 strides-2 projections and the VGG-64 pooled layer): microseconds
per launch from hipEvents over back-to-back launches, and the fraction of the measured f32 matrix peak (155 TFLOP/s,
2 FLOP per MAC).  Per network: images/s of nets.Model(cf, spec).predict on the 'bf' and 'tf' checkpoints (CIFAR-10
ResNet, nres 3), device-resident input, both kernel families.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qnn_amd import _abi, engine, nets  # noqa: E402

F32 = np.float32
PEAK = 155e12
LAYERS = [  # name, H, cin, cout, k, stride, pool
    ("16-16 32x32", 32, 16, 16, 3, 1, 1), ("16-32 s2", 32, 16, 32, 3, 2, 1), ("32-32 16x16", 16, 32, 32, 3, 1, 1),
    ("32-64 s2", 16, 32, 64, 3, 2, 1), ("64-64 8x8", 8, 64, 64, 3, 1, 1), ("1x1 16-32 s2", 32, 16, 32, 1, 2, 1),
    ("1x1 32-64 s2", 16, 32, 64, 1, 2, 1), ("VGG 64-64 32x32 pool", 32, 64, 64, 3, 1, 2)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def bench_layer(n, H, cin, cout, k, stride, pool, reps):
    rng = np.random.default_rng(0)
    x = torch.as_tensor(rng.standard_normal((n, H, H, cin)).astype(F32)).cuda()
    op = {"op": "conv", "kind": "binary", "kernel": rng.uniform(-1, 1, (k, k, cin, cout)).astype(F32), "bias": None,
          "strides": (stride, stride), "padding": "same"}
    w = engine._prepack(op, _abi.STORE_F32, torch.device("cuda"), stride=stride, same_pad=True)
    inv = torch.ones(cout, device="cuda")
    shift = torch.zeros(cout, device="cuda")
    Ho = -(-H // stride)
    out = torch.empty((n, Ho // pool, Ho // pool, cout), device="cuda")
    row = {}
    for impl, key in ((_abi.IMPL_AUTO, "f32act"), (_abi.IMPL_VALU, "generic")):
        _abi.set_conv_impl(impl)
        call = lambda: _abi.conv2d(w, x, _abi.STORE_F32, 0, n, H, H, inv, shift, _abi.FN_LEAKY_RELU, 0, pool,
                                   _abi.STORE_F32, out=out)
        call()
        row[key + "_kernel"] = _abi.last_kernel()
        us = timed(call, reps if key == "f32act" else max(2, reps // 10))
        row[key + "_us"] = round(us, 2)
        row[key + "_peak_frac"] = round(2.0 * n * Ho * Ho * k * k * cin * cout / (us * 1e-6) / PEAK, 4)
    _abi.set_conv_impl(_abi.IMPL_AUTO)
    return row


def bench_predict(code, n, reps):
    spec = nets.spec_from_keras_npz(os.path.join(ROOT, "tests", "golden", "resnet3_full_%s.npz" % code))
    cf = nets.Config(network_type="full-qnn", architecture="RESNET", nres=3, dim=32)
    x = torch.as_tensor(nets.synthetic_images(cf, 4 * n, 1)).cuda()
    row = {}
    for impl, key in ((_abi.IMPL_AUTO, "f32act"), (_abi.IMPL_VALU, "generic")):
        _abi.set_conv_impl(impl)
        model = nets.Model(cf, spec)
        xs = x if key == "f32act" else x[:n]
        us = timed(lambda: model.predict(xs, batch_size=n), reps if key == "f32act" else 1)
        row[key + "_img_s"] = round(len(xs) / (us * 1e-6))
    _abi.set_conv_impl(_abi.IMPL_AUTO)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"n": a.n, "peak_tflops": PEAK / 1e12, "layers": {}, "predict": {}}
    for name, H, cin, cout, k, stride, pool in LAYERS:
        res["layers"][name] = r = bench_layer(a.n, H, cin, cout, k, stride, pool, a.reps)
        print(name, r, flush=True)
    for code in ("bf", "tf"):
        res["predict"][code] = r = bench_predict(code, a.n, max(2, a.reps // 4))
        print("predict", code, r, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
