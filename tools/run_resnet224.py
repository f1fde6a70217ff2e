#!/usr/bin/env python3
"""BASELINE config 5: synthetic ImageNet-224 ResNet (nres=10, pfilt=1) full-qnn 4/4 through GraphModel.
Environment: B (batch, 64), CHECK (1: one image against the oracle first), WBITS / ABITS (other full-qnn widths, e.g. 8 / 8),
DIM / NRES (e.g. DIM=32 NRES=3: the CIFAR ResNet-20), PREDICT=1 (time nets.Model(...).predict on IMAGES resident images, the
product call with its hipGraph lanes, instead of GraphModel), FUSE_TAIL=0 (with PREDICT=1: the classifier tail as three
launches instead of one)."""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
pkg = importlib.import_module("quantizedneuralnetworks-keras-tensorflow_amd")
nets, engine = pkg.nets, pkg.engine
from oracle import qnn_oracle as O

cf = nets.baseline_config(4)
if any(k in os.environ for k in ("WBITS", "ABITS", "DIM", "NRES")):
    dim = int(os.environ.get("DIM", cf.dim))
    cf = nets.Config(network_type="full-qnn", wbits=int(os.environ.get("WBITS", cf.wbits)), abits=int(os.environ.get("ABITS", cf.abits)),
                     architecture="RESNET", nres=int(os.environ.get("NRES", cf.nres)), dim=dim, channels=cf.channels,
                     classes=cf.classes if dim == cf.dim else 10)
spec = nets.build_spec(cf, nets.SEED_BASE + 4)
if os.environ.get("PREDICT") == "1":
    B = int(os.environ.get("B", "64"))
    n = int(os.environ.get("IMAGES", str(8 * B)))
    m = nets.Model(cf, spec)
    m.engine.kernel_log = []
    m.engine.fuse_tail = os.environ.get("FUSE_TAIL", "1") == "1"
    x = torch.as_tensor(nets.synthetic_images(cf, n, 6)).cuda()
    m.engine(x[:min(B, 4)])
    kernels = sorted(set(m.engine.kernel_log))
    m.engine.kernel_log = None
    for _ in range(2):
        m.predict(x, batch_size=B)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(5):
        t0 = time.perf_counter()
        m.predict(x, batch_size=B)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    print(json.dumps({"workload": "resnet dim %d nres %d w%da%d predict" % (cf.dim, cf.nres, cf.wbits, cf.abits), "batch": B,
                      "images": n, "ms": round(best * 1e3, 2), "images_per_s": round(n / best, 1), "kernels": kernels}))
    sys.exit(0)
model = engine.GraphModel(spec)
B = int(os.environ.get("B", "64"))
if os.environ.get("CHECK", "1") == "1":
    x1 = nets.synthetic_images(cf, 1, 5)
    t0 = time.time(); want = O.run_spec(spec, x1, float_conv="device"); t_or = time.time() - t0
    got = model(torch.as_tensor(x1).cuda()).cpu().numpy()
    print(json.dumps({"check": "resnet224 N=1 vs oracle", "max_abs_diff": float(np.abs(got - want).max()),
                      "oracle_s": round(t_or, 1)}))
x = torch.as_tensor(nets.synthetic_images(cf, B, 6)).cuda()
for _ in range(2):
    y = model(x)
torch.cuda.synchronize()
t0 = time.perf_counter()
reps = 3
for _ in range(reps):
    y = model(x)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / reps
print(json.dumps({"workload": "imagenet224_resnet10_w4a4", "batch": B, "ms": round(dt * 1e3, 2),
                  "images_per_s": round(B / dt, 1), "max_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2)}))
