"""The ResNet classifier tail in one launch (qnn_avgpool_dense_softmax_forward, engine fuse_tail) against the three launches
it replaces -- qnn_avgpool_packed_f32 -> qnn_dense_forward on a QNN_STORE_F32 handle -> qnn_softmax_f32 -- bit for bit
(torch.equal, no tolerance): at the call level over stores, bit widths, shapes, batch sizes, class counts and dense
kinds; through ResidualFusedModel / GraphModel with fuse_tail on and off; and through Model.predict (hipGraph lanes).
The three launches themselves are held against integer / float64 references by test_gpu_tail.py."""
import os
import zlib

import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine, nets
import tail_cases as T

pytestmark = pytest.mark.gpu
F32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
I4, I8, BIN = _abi.STORE_I4, _abi.STORE_I8, _abi.STORE_BIN
CIFAR, TWO, CROP, INET, ODD = (8, 8, 8, 64), (16, 16, 8, 16), (17, 19, 8, 32), (56, 56, 8, 64), (8, 8, 8, 24)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _codes(rng, N, H, W, C, store, bits, fill):
    lo, hi = T.code_range(store, bits)
    if fill == "min":
        return np.full((N, H, W, C), lo, np.int8)
    if fill == "max":
        return np.full((N, H, W, C), hi, np.int8)
    c = T.random_codes(rng, (N, H, W, C), store, bits)
    if N:                                   # the extremes inside a random map: one all-minimum and one all-maximum channel
        c[0, :, :, 0], c[-1, :, :, C - 1] = lo, hi
    return c


def _weights(rng, K, classes, kind, nb, bias):
    kernel = rng.uniform(-1, 1, (K, classes)).astype(F32)
    b = dev(rng.normal(0, 0.5, classes).astype(F32)) if bias else None
    wkind = {"quantized": _abi.W_QUANT, "binary": _abi.W_BINARY, "ternary": _abi.W_TERNARY}[kind]
    return _abi.Weights(wkind, nb, 1.0, dev(kernel), b, 1, True, _abi.STORE_F32)


def _three_launches(w, xp, store, bits, N, H, W, C, size, softmax=True):
    pooled = _abi.avgpool_packed(xp, store, bits, N, H, W, C, size)
    logits = _abi.dense(w, pooled.reshape(N, -1), _abi.STORE_F32, 0, N)
    return logits, (_abi.softmax(logits) if softmax else logits)


# (shape, store, bits, N, classes, dense kind, nb, bias, softmax, fill): every value of every axis of the issue's table at
# least once; K = 3136 with 70 classes; N = 257 = more images than one workgroup takes, and no multiple of its share
CASES = [
    (CIFAR, I4, 4, 257, 10, "quantized", 4, False, True, "random"),
    (CIFAR, I4, 4, 3, 10, "quantized", 4, True, True, "min"),
    (CIFAR, I4, 4, 3, 10, "quantized", 8, False, True, "max"),
    (CIFAR, I4, 2, 257, 10, "quantized", 8, True, False, "random"),
    (CIFAR, I4, 1, 3, 70, "binary", 1, False, True, "random"),
    (CIFAR, I4, 4, 1, 1, "ternary", 1, True, True, "random"),
    (CIFAR, I4, 4, 0, 10, "quantized", 4, False, True, "random"),
    (CIFAR, I8, 8, 257, 10, "quantized", 8, False, True, "random"),
    (CIFAR, I8, 8, 3, 70, "quantized", 4, True, True, "min"),
    (CIFAR, BIN, 1, 257, 10, "binary", 1, True, True, "random"),
    (CIFAR, BIN, 1, 1, 10, "binary", 1, False, True, "max"),
    (CIFAR, BIN, 1, 3, 1, "ternary", 1, False, False, "min"),
    (TWO, I4, 4, 257, 10, "quantized", 4, True, True, "random"),
    (TWO, I4, 2, 3, 70, "ternary", 1, False, True, "random"),
    (TWO, I8, 8, 1, 10, "binary", 1, True, False, "random"),
    (TWO, BIN, 1, 3, 10, "binary", 1, False, True, "random"),
    (CROP, I4, 4, 3, 10, "quantized", 4, False, True, "random"),
    (CROP, I4, 1, 257, 1, "binary", 1, True, True, "random"),
    (CROP, I8, 8, 3, 70, "quantized", 8, True, True, "random"),
    (CROP, BIN, 1, 1, 10, "ternary", 1, False, True, "random"),
    (INET, I4, 4, 3, 70, "quantized", 4, False, True, "random"),
    (INET, I4, 4, 1, 70, "quantized", 4, True, True, "max"),
    (INET, I4, 2, 2, 70, "ternary", 1, False, False, "random"),
    (INET, I8, 8, 1, 70, "quantized", 8, True, True, "random"),
    (INET, BIN, 1, 2, 70, "binary", 1, False, True, "random"),
    (ODD, I8, 8, 257, 10, "quantized", 8, False, True, "random"),
    (ODD, I8, 8, 3, 70, "quantized", 4, True, True, "max"),
    (ODD, I8, 8, 1, 1, "binary", 1, False, False, "random"),
    # beyond the table: K % 4 != 0 (the scalar branch of the dense order), a window smaller than the 8 lanes of a pooling
    # task, an un-pooled map
    ((8, 8, 8, 7), BIN, 1, 5, 10, "binary", 1, True, True, "random"),
    ((6, 6, 2, 9), I4, 4, 5, 10, "quantized", 4, False, True, "random"),
    ((3, 5, 1, 12), I8, 8, 5, 3, "quantized", 8, True, True, "random"),
]


def _id(c):
    (H, W, s, C), store, bits, N, classes, kind, nb, bias, sm, fill = c
    return "%dx%dx%d_p%d-%s%d-N%d-u%d-%s%d%s-%s-%s" % (H, W, C, s, T.STORE_NAME[store], bits, N, classes, kind[0], nb,
                                                      "+b" if bias else "", "sm" if sm else "logits", fill)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_fused_tail_equals_the_three_launches(case):
    (H, W, size, C), store, bits, N, classes, kind, nb, bias, sm, fill = case
    rng = np.random.default_rng(zlib.crc32(_id(case).encode()))
    K = (H // size) * (W // size) * C
    w = _weights(rng, K, classes, kind, nb, bias)
    codes = _codes(rng, N, H, W, C, store, bits, fill)
    words = T.pack_words(codes.reshape(-1, C), store).view(np.int32)
    xp = torch.zeros((N * H * W + 1, words.shape[1]), dtype=torch.int32, device="cuda")     # N = 0: still a pointer
    if N:
        xp[:N * H * W] = dev(words)
    logits = torch.full((N, classes), float("nan"), device="cuda") if sm else None
    got = _abi.avgpool_dense_softmax(w, xp, store, bits, N, H, W, C, size, softmax=sm, logits=logits)
    assert tuple(got.shape) == (N, classes) and got.dtype == torch.float32
    if N == 0:
        return
    assert _abi.last_kernel() == ("tail_avg_dense_softmax" if sm else "tail_avg_dense")
    want_logits, want = _three_launches(w, xp, store, bits, N, H, W, C, size, sm)
    torch.cuda.synchronize()
    assert torch.equal(got, want), (got - want).abs().max().item()
    if sm:
        assert torch.equal(logits, want_logits)


def test_bn_behind_the_dense_layer_as_qnn_dense_forward_applies_it():
    rng = np.random.default_rng(5)
    H, W, size, C = CIFAR
    w = _weights(rng, 64, 10, "quantized", 4, True)
    inv, shift = dev(rng.uniform(0.5, 2, 10).astype(F32)), dev(rng.normal(0, 1, 10).astype(F32))
    xp = dev(T.pack_words(_codes(rng, 9, H, W, C, I4, 4, "random").reshape(-1, C), I4).view(np.int32))
    got = _abi.avgpool_dense_softmax(w, xp, I4, 4, 9, H, W, C, size, bn_inv=inv, bn_shift=shift)
    pooled = _abi.avgpool_packed(xp, I4, 4, 9, H, W, C, size)
    want = _abi.softmax(_abi.dense(w, pooled.reshape(9, -1), _abi.STORE_F32, 0, 9, inv, shift))
    assert torch.equal(got, want)


def test_declines_leave_the_three_launch_form_and_the_kernel_name():
    rng = np.random.default_rng(6)
    H, W, size, C = CIFAR
    w = _weights(rng, 64, 10, "quantized", 4, False)
    codes = _codes(rng, 2, H, W, C, I4, 4, "random")
    xp = dev(T.pack_words(codes.reshape(-1, C), I4).view(np.int32))
    _abi.avgpool_dense_softmax(w, xp, I4, 4, 2, H, W, C, size)
    assert _abi.last_kernel() == "tail_avg_dense_softmax"
    _abi.dense(w, torch.zeros(2, 64, device="cuda"), _abi.STORE_F32, 0, 2)
    before = _abi.last_kernel()
    assert before == "dense_f32"
    # ternary bit planes
    t2 = dev(T.pack_words(np.sign(codes).reshape(-1, C), _abi.STORE_T2).view(np.int32))
    with pytest.raises(_abi.QnnUnsupported):
        _abi.avgpool_dense_softmax(w, t2, _abi.STORE_T2, 1, 2, H, W, C, size)
    # a dense handle prepacked for packed int4 input
    w4 = _abi.Weights(_abi.W_QUANT, 4, 1.0, dev(rng.uniform(-1, 1, (64, 10)).astype(F32)), None, 1, True, I4)
    with pytest.raises(_abi.QnnUnsupported):
        _abi.avgpool_dense_softmax(w4, xp, I4, 4, 2, H, W, C, size)
    # an activation behind the dense layer
    with pytest.raises(_abi.QnnUnsupported):
        _abi.avgpool_dense_softmax(w, xp, I4, 4, 2, H, W, C, size, fn=_abi.FN_BINARY_TANH)
    # more averages per image than the kernel keeps in LDS (64 KiB): 17 x 17 x 64 floats
    big = _weights(rng, 17 * 17 * 64, 2, "binary", 1, False)
    xb = torch.zeros((17 * 17, 8), dtype=torch.int32, device="cuda")
    with pytest.raises(_abi.QnnUnsupported):
        _abi.avgpool_dense_softmax(big, xb, I4, 4, 1, 17, 17, 64, 1)
    assert _abi.last_kernel() == before
    # not a decline but an error: a dense layer of another width
    with pytest.raises(_abi.QnnError) as e:
        _abi.avgpool_dense_softmax(w, xp, I4, 4, 2, H, W, 32, size)
    assert not isinstance(e.value, _abi.QnnUnsupported)


# ---- engines ---------------------------------------------------------------------------------------------------------
def _resnet(nt, wb, ab):
    cf = nets.Config(network_type=nt, wbits=wb, abits=ab, architecture="RESNET", nres=1, dim=32)
    return cf, nets.build_spec(cf, 31)


def _trained(code, wb, ab):
    return nets.Config(dim=32), nets.spec_from_keras_npz(os.path.join(GOLD, "resnet3_full_%s.npz" % code), wb, ab)


ENGINE_SPECS = {"qnn44": lambda: _resnet("full-qnn", 4, 4), "qnn88": lambda: _resnet("full-qnn", 8, 8),
                "bnn": lambda: _resnet("full-bnn", 1, 1), "trained44": lambda: _trained("44", 4, 4),
                "trained_bb": lambda: _trained("bb", None, None)}


def _on_off(m, x):
    """The model's forward with the tail fused and as three launches: the outputs and the last kernel name of each."""
    outs, last = [], []
    assert m.fuse_tail is True
    for fuse in (True, False):
        m.fuse_tail = fuse
        outs.append(m(x))
        torch.cuda.synchronize()
        last.append(_abi.last_kernel())
    m.fuse_tail = True
    return outs, last


@pytest.mark.parametrize("name", sorted(ENGINE_SPECS))
def test_residual_engine_fuses_the_tail_bit_for_bit(name):
    cf, spec = ENGINE_SPECS[name]()
    x = dev(nets.synthetic_images(cf, 5, 12))
    (on, off), last = _on_off(engine.ResidualFusedModel(spec), x)
    assert torch.equal(on, off)
    assert last == ["tail_avg_dense_softmax", "dense_f32"], last
    # a spec without the softmax op: the dense layer is its last op
    (on, off), last = _on_off(engine.ResidualFusedModel(spec[:-1]), x)
    assert torch.equal(on, off)
    assert last == ["tail_avg_dense", "dense_f32"], last


def test_full_tnn_gives_the_same_bits_either_way():
    """Ternary activations.  The residual engine stores the last ternary activation as sign / mask planes (QNN_STORE_T2)
    only where a ternary contraction reads it; behind the average pool alone it packs int4 codes {-1, 0, 1}, and the tail
    then fuses like any int4 tail.  Either way the two forms agree bit for bit and nothing is raised."""
    cf, spec = _resnet("full-tnn", 1, 1)
    x = dev(nets.synthetic_images(cf, 5, 12))
    (on, off), last = _on_off(engine.ResidualFusedModel(spec), x)
    assert torch.equal(on, off)
    assert last[1] == "dense_f32" and last[0] in ("tail_avg_dense_softmax", "dense_f32"), last


def test_a_declined_tail_falls_back_silently():
    """A tail the library declines (16 x 16 x 64 averages + 10 logits per image: over the 64 KiB LDS cap) runs as three
    launches, as before; the decline is remembered, so the library is asked once."""
    cf = nets.Config(network_type="full-qnn", wbits=4, abits=4, architecture="RESNET", nres=1, dim=64)
    spec = [dict(op) for op in nets.build_spec(cf, 31)]
    pool = next(op for op in spec if op["op"] == "avgpool")
    dense = next(op for op in spec if op["op"] == "dense")
    pool["size"] = 1
    dense["kernel"] = np.random.default_rng(3).uniform(-1, 1, (16 * 16 * 64, cf.classes)).astype(F32)
    x = dev(nets.synthetic_images(cf, 3, 12))
    m = engine.ResidualFusedModel(spec)
    (on, off), last = _on_off(m, x)
    assert torch.equal(on, off)
    assert last == ["dense_f32", "dense_f32"], last           # avg-pool and softmax record no kernel name of their own
    assert m.graph.tail_no == {len(spec) - 1}


def test_graph_model_fuses_the_tail_bit_for_bit():
    cf, spec = _resnet("full-qnn", 4, 4)
    x = dev(nets.synthetic_images(cf, 5, 12))
    (on, off), last = _on_off(engine.GraphModel(spec), x)
    assert torch.equal(on, off)
    assert last == ["tail_avg_dense_softmax", "dense_f32"], last


def test_predict_replays_the_fused_tail_from_hipgraphs():
    """2 full batches of 8 (hipGraph lanes, the tail's output is the lane's static output) and a ragged tail of 3."""
    cf, spec = _resnet("full-qnn", 4, 4)
    x = dev(nets.synthetic_images(cf, 19, 13))
    m = nets.Model(cf, spec)
    assert isinstance(m.engine, engine.ResidualFusedModel) and m.engine.fuse_tail
    got = m.predict(x, batch_size=8)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (19, cf.classes)
    eager = engine.ResidualFusedModel(spec)
    for lo in (0, 8, 16):
        want = eager(x[lo:lo + 8])
        assert _abi.last_kernel() == "tail_avg_dense_softmax"
        assert torch.equal(got[lo:lo + 8], want), lo
