"""Keras pooling on the GPU (csrc/qnn_pool.hip, include/qnn_abi_pool.h): every store x mode x case x value set of
pool_cases.py against its numpy reference -- the maxima as raw packed words (which also pins the spare bits of a pixel's
last word), the averages bit for bit -- the four layer classes, and one small network with a new-form max-pool and a
global average on every engine."""
import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi, engine, nets
from oracle import qnn_oracle as O

import pool_cases as P

pytestmark = pytest.mark.gpu
F32 = np.float32
STORE = {"bin": _abi.STORE_BIN, "i4": _abi.STORE_I4, "i8": _abi.STORE_I8, "f32": _abi.STORE_F32}
MODE = {"max": _abi.POOL_MAX, "avg": _abi.POOL_AVG}


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # (a copy: the shared cases are read-only)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- the kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["max", "avg"])
@pytest.mark.parametrize("kind", ["bin", "i4", "i8", "f32"])
def test_pool_kernels_against_the_reference(kind, mode):
    store = STORE[kind]
    for gi, g in enumerate(P.GEOMS):
        N, H, W, size, strides, padding = P.geom(g)
        for C, bits in P.BITS[kind]:
            for vset in P.VALUE_SETS:
                what = (g, C, bits, vset)
                x, want = P.values(gi, kind, C, bits, vset), P.expected(gi, kind, C, bits, vset, mode)
                xin = dev(x) if kind == "f32" else _abi.pack(dev(x), C, _abi.FN_GRID, bits, store)
                y, Ho, Wo = _abi.pool2d(xin, store, bits, N, H, W, C, MODE[mode], size, strides, padding == "same")
                assert _abi.last_kernel() == "pool_%s_%s" % (mode, kind), what
                assert (Ho, Wo) == want.shape[1:3], what
                if mode == "max" and kind != "f32":
                    # the raw words of the packed reference: codes, layout and the zero bits behind the last channel
                    assert y.dtype == torch.int32 and torch.equal(y, _abi.pack(dev(want), C, _abi.FN_GRID, bits, store)), what
                else:
                    assert y.dtype == torch.float32 and same_bits(host(y), want), what


@pytest.mark.parametrize("kind,C,bits", [("bin", 33, 1), ("bin", 70, 1), ("i4", 9, 4), ("i4", 7, 3), ("i8", 5, 8), ("i8", 1, 5)])
def test_spare_bits_of_the_last_word_are_written_as_pack_writes_them(kind, C, bits):
    """Whatever the input holds behind channel C - 1, the output holds zeros there (qnn_pack_f32's form), and the
    average does not read those fields."""
    store, gi = STORE[kind], 7                        # 3 x 8 x 8, window 3, strides 2, 'same'
    N, H, W, size, strides, padding = P.geom(P.GEOMS[gi])
    x = P.values(gi, kind, C, bits, "random")
    xp = _abi.pack(dev(x), C, _abi.FN_GRID, bits, store)
    used = (C - (xp.shape[1] - 1) * _abi.per_word(store)) * (32 // _abi.per_word(store))
    dirty = xp.clone()
    dirty[:, -1] |= torch.tensor(np.array([(0xFFFFFFFF << used) & 0xFFFFFFFF], np.uint32).view(np.int32)[0]).cuda()
    assert not torch.equal(dirty, xp)
    for mode in ("max", "avg"):
        want = P.expected(gi, kind, C, bits, "random", mode)
        y, _, _ = _abi.pool2d(dirty, store, bits, N, H, W, C, MODE[mode], size, strides, True)
        if mode == "max":
            assert torch.equal(y, _abi.pack(dev(want), C, _abi.FN_GRID, bits, store))
        else:
            assert same_bits(host(y), want)


def test_an_unaligned_tensor_takes_the_one_word_path():
    """Words per pixel divisible by 4 but a base address that is not 16-byte aligned: same words."""
    gi, C = 7, 64
    N, H, W, size, strides, padding = P.geom(P.GEOMS[gi])
    x, want = P.values(gi, "i4", C, 4, "random"), P.expected(gi, "i4", C, 4, "random", "max")
    xp = _abi.pack(dev(x), C, _abi.FN_GRID, 4, _abi.STORE_I4)
    buf = torch.zeros(xp.numel() + 1, dtype=torch.int32, device="cuda")
    off = buf[1:].view(xp.shape)
    off.copy_(xp)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    y, _, _ = _abi.pool2d(off, _abi.STORE_I4, 4, N, H, W, C, _abi.POOL_MAX, size, strides, True)
    assert torch.equal(y, _abi.pack(dev(want), C, _abi.FN_GRID, 4, _abi.STORE_I4))


def test_an_empty_batch_and_the_refusals():
    y, Ho, Wo = _abi.pool2d(torch.zeros((0, 8, 8, 4), device="cuda"), _abi.STORE_F32, 0, 0, 8, 8, 4, _abi.POOL_AVG, 3, 2, True)
    assert tuple(y.shape) == (0, 4, 4, 4)
    with pytest.raises(_abi.QnnError, match="larger than"):
        _abi.pool2d(torch.zeros((1, 2, 2, 4), device="cuda"), _abi.STORE_F32, 0, 1, 2, 2, 4, _abi.POOL_MAX, 3)
    with pytest.raises(_abi.QnnUnsupported):
        _abi.pool2d(torch.zeros((4, 2), dtype=torch.int32, device="cuda"), _abi.STORE_T2, 1, 1, 2, 2, 8, _abi.POOL_MAX, 2)


def test_layer_classes_on_float32():
    for gi, g in enumerate(P.GEOMS):
        N, H, W, size, strides, padding = P.geom(g)
        for C in P.CHANNELS["f32"]:
            x = P.values(gi, "f32", C, 0, "random")
            for cls, mode in ((qnn_amd.MaxPooling2D, "max"), (qnn_amd.AveragePooling2D, "avg")):
                layer = cls(pool_size=size, strides=strides, padding=padding)
                y = host(layer(dev(x)))
                assert same_bits(y, P.expected(gi, "f32", C, 0, "random", mode)), (g, C, mode)
                assert layer.compute_output_shape(x.shape) == y.shape
            if g[3] == "whole" and padding == "valid":
                for cls, mode in ((qnn_amd.GlobalMaxPooling2D, "max"), (qnn_amd.GlobalAveragePooling2D, "avg")):
                    y = host(cls()(dev(x)))
                    assert same_bits(y, P.global_ref(x, mode)) and cls().compute_output_shape(x.shape) == y.shape
                    assert same_bits(y, P.expected(gi, "f32", C, 0, "random", mode).reshape(N, C))


# ---- one small network ----------------------------------------------------------------------------------------------------
def _bn(rng, n, var):
    return dict(op="bn", eps=1e-4, gamma=rng.uniform(0.5, 1.5, n).astype(F32), beta=(rng.standard_normal(n) * 0.3).astype(F32),
                mean=(rng.standard_normal(n) * 0.1 * np.sqrt(var)).astype(F32), var=(var * rng.uniform(0.8, 1.25, n)).astype(F32))


def _net(pool):
    """9 x 9 x 8 float32 -> QuantizedConv2D 8 -> 8 (4 bits, 'same'), BN, quantized_tanh(4) -> `pool` -> a second group ->
    global average -> dense 8 -> 10 -> softmax."""
    rng = np.random.default_rng(2024)
    conv = lambda: {"op": "conv", "kind": "quantized", "nb": 4, "kernel": rng.uniform(-1, 1, (3, 3, 8, 8)).astype(F32),
                    "bias": (rng.standard_normal(8) * 0.05).astype(F32), "strides": (1, 1), "padding": "same"}
    q4 = lambda: {"op": "act", "fn": "quantized_tanh", "nb": 4}
    return [conv(), _bn(rng, 8, 72 * 0.1), q4(), pool, conv(), _bn(rng, 8, 72 * 0.12), q4(), {"op": "globalavgpool"},
            {"op": "dense", "kind": "quantized", "nb": 4, "kernel": rng.uniform(-1, 1, (8, 10)).astype(F32),
             "bias": (rng.standard_normal(10) * 0.05).astype(F32)}, {"op": "softmax"}]


NEW_POOL = {"op": "maxpool", "size": 3, "strides": (2, 2), "padding": "same"}


def _images(n):
    rng = np.random.default_rng(7)
    return (rng.integers(0, 256, (n, 9, 9, 8)).astype(F32) / F32(255)).astype(F32)


def _composed_reference(spec, x):
    """The oracle on the sub-chains around the two new ops, the numpy reference for the ops themselves."""
    a = O.run_spec(spec[:3], x, float_conv="device")
    assert a.shape == (x.shape[0], 9, 9, 8)
    p = P.pool2d_ref(a, "max", 3, (2, 2), "same")
    assert p.shape == (x.shape[0], 5, 5, 8)
    b = O.run_spec(spec[4:7], p)
    return O.run_spec(spec[8:], P.global_ref(b, "avg")), O.run_spec(spec[8:9], P.global_ref(b, "avg"))


def within(got, want):
    r = float((np.abs(got.astype(np.float64) - want) / (1e-5 * np.maximum(1.0, np.abs(want)))).max())
    assert r <= 1.0, "max |d| / (1e-5 * max(1, |y|)) = %.3g" % r


def test_a_network_with_a_new_form_max_pool_on_every_engine():
    spec, x = _net(NEW_POOL), _images(6)
    want, want_logits = _composed_reference(spec, x)
    xd = dev(x)
    graph = engine.GraphModel(spec)
    graph.kernel_log = []
    got = {"GraphModel": host(graph(xd))}
    # the activation was packed for the pool and the pool ran on the codes: it never existed in float32 behind the clip
    assert graph.kernel_log == ["pool_max_i4", "pool_avg_i4"], graph.kernel_log
    res = engine.ResidualFusedModel(spec, first_layer="exact")
    res.kernel_log = []
    got["ResidualFusedModel"] = host(res(xd))
    assert [k for k in res.kernel_log if k.startswith("pool")] == ["pool_max_i4", "pool_avg_i4"], res.kernel_log
    got["LayerModel"] = host(engine.LayerModel(spec)(xd))
    with pytest.raises(_abi.NotFusable):
        engine.FusedModel(spec, first_layer="exact")
    model = nets.Model(nets.Config(dim=9, channels=8), spec, first_layer="exact")
    assert type(model.engine).__name__ == "ResidualFusedModel"
    got["nets.Model"] = model.predict(x, batch_size=4)
    pipe = engine.Pipelined(engine.GraphModel(spec), lanes=2, batch_size=4)       # one captured replay + a ragged tail of 2
    got["Pipelined"] = host(pipe(xd))
    for name, y in got.items():
        assert y.shape == (6, 10), name
        within(y, want)
        np.testing.assert_allclose(y, got["GraphModel"], atol=1e-6, err_msg=name)      # softmax: exp differs in the last ulp
    # the logits in front of the softmax agree bit for bit between the engines
    logits = {cls.__name__: host(cls(spec[:-1], **kw)(xd)) for cls, kw in
              ((engine.GraphModel, {}), (engine.ResidualFusedModel, {"first_layer": "exact"}), (engine.LayerModel, {}))}
    for name, y in logits.items():
        within(y, want_logits)
        np.testing.assert_array_equal(y, logits["GraphModel"], err_msg=name)


def test_the_old_form_goes_the_way_it_went():
    """The same network with the size-only max-pool: the kernels of the parent commit, as literals.  GraphModel keeps no
    log of its contractions (the parent ignored `kernel_log` altogether): its list holds new-form pools only."""
    spec, x = _net({"op": "maxpool", "size": 2}), _images(3)
    assert not engine._new_pool(spec[3])
    graph = engine.GraphModel(spec)
    graph.kernel_log = []
    y = host(graph(dev(x)))
    assert graph.kernel_log == ["pool_avg_i4"], graph.kernel_log       # the global average is the network's only new op
    graph = engine.GraphModel(spec[:7])                               # ... and without it: what the parent logged
    graph.kernel_log = []
    graph(dev(x))
    assert graph.kernel_log == []
    res = engine.ResidualFusedModel(spec[:7], first_layer="exact")
    res.kernel_log = []
    z = host(res(dev(x)))
    assert res.kernel_log == PARENT_KERNELS, res.kernel_log
    np.testing.assert_array_equal(z, O.run_spec(spec[:7], x, float_conv="device"))
    a = O.run_spec(spec[:7], x, float_conv="device")
    within(y, O.run_spec(spec[8:], P.global_ref(a, "avg")))


# what ResidualFusedModel(_net(old-form pool)[:7]).kernel_log holds on the parent commit
PARENT_KERNELS = ["generic", "generic"]
