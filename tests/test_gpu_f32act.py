"""The float32-activation convolution on the f32 matrix pipe (csrc/qnn_f32act.hip) and the fused LeakyReLU epilogue
(QNN_FN_LEAKY_RELU), layer by layer and through the networks whose activations stay float32.

Bar: bit-identical to k_conv_generic (qnn_set_conv_impl(1)) and to the oracle's device-order FMA chain followed by the
epilogue in numpy; networks bit-identical to the VALU-only engine and within the LeakyReLU network tolerance of the
oracle."""
import os
import zlib

import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine, nets
from oracle import qnn_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WKINDS = [("binary", None), ("ternary", None), ("quantized", 2), ("quantized", 4), ("quantized", 8), ("float", None)]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


class valu_only:
    """qnn_set_conv_impl(1): the VALU kernels and k_conv_generic only."""

    def __enter__(self):
        _abi.set_conv_impl(_abi.IMPL_VALU)

    def __exit__(self, *a):
        _abi.set_conv_impl(_abi.IMPL_AUTO)


def leaky(v):
    return np.where(v >= 0, v, (v * F32(0.3)).astype(F32)).astype(F32)


def _qkernel(op):
    k = op["kernel"]
    if op["kind"] == "binary":
        return O.binarize(k)
    if op["kind"] == "ternary":
        return O._ternarize(k)
    if op["kind"] == "quantized":
        return O.quantize(k, op["nb"])
    return k


def _oracle(x, op, inv, shift, res, post, fn, pool, act_bits=0):
    st = tuple(op["strides"])
    v = O.conv2d_device_order(x, _qkernel(op), st, "same")
    if op.get("bias") is not None:
        v = (v + op["bias"]).astype(F32)
    if inv is not None:
        v = ((v * inv).astype(F32) + shift).astype(F32)
    if res is not None:
        v = ((res + v).astype(F32) * F32(post)).astype(F32)
    if fn == _abi.FN_LEAKY_RELU:
        v = leaky(v)
    elif fn == _abi.FN_BINARY_TANH:
        v = O.binary_tanh(v)
    elif fn == _abi.FN_QUANTIZED_TANH:
        v = O.quantized_tanh(v, act_bits)
    if pool == 2:
        N, H, W, C = v.shape
        w = v[:, :H // 2 * 2, :W // 2 * 2].reshape(N, H // 2, 2, W // 2, 2, C)
        v = np.maximum(np.maximum(np.maximum(w[:, :, 0, :, 0], w[:, :, 0, :, 1]), w[:, :, 1, :, 0]), w[:, :, 1, :, 1])
    return v


def _case(idx, N, H, W, cin, cout, k, stride):
    rng = np.random.default_rng(zlib.crc32(repr((idx, N, H, W, cin, cout, k, stride)).encode()))
    wkind, nb = WKINDS[idx % len(WKINDS)]
    x = leaky(rng.standard_normal((N, H, W, cin)).astype(F32))       # negative, off-grid activations
    op = {"op": "conv", "kind": wkind, "kernel": rng.uniform(-1, 1, (k, k, cin, cout)).astype(F32),
          "bias": (rng.standard_normal(cout) * 0.1).astype(F32) if idx % 2 == 0 else None,
          "strides": (stride, stride), "padding": "same"}
    if nb:
        op["nb"] = nb
    inv = shift = None
    if idx % 3 != 2:
        var = F32(k * k * cin * 0.3)
        bn = dict(eps=1e-3, gamma=rng.uniform(-1.5, 1.5, cout).astype(F32), beta=(rng.standard_normal(cout) * 0.3).astype(F32),
                  mean=(rng.standard_normal(cout) * 0.1).astype(F32), var=(var * rng.uniform(0.8, 1.25, cout)).astype(F32))
        inv, shift = engine.bn_constants(bn)
    return rng, op, x, inv, shift


def _run(op, x, inv, shift, fn, pool, res=None, post=1.0, act_bits=0):
    N, H, W, C = x.shape
    w = engine._prepack(op, _abi.STORE_F32, torch.device("cuda"), stride=op["strides"][0], same_pad=True)
    kw = {}
    if res is not None:
        kw = dict(res=dev(res), res_store=_abi.STORE_F32, res_bits=0, post_scale=post)
    y, _, _ = _abi.conv2d(w, dev(x), _abi.STORE_F32, 0, N, H, W, None if inv is None else dev(inv),
                          None if shift is None else dev(shift), fn, act_bits, pool, _abi.STORE_F32, **kw)
    kern = _abi.last_kernel()
    return host(y), kern


GEOMS = [(3, 1), (3, 2), (1, 2)]
SHAPES = [(1, 9, 13), (3, 16, 16), (1, 12, 7), (3, 11, 20)]          # odd / even H, W; W not a multiple of 16
CASES = [(cin, cout, k, s) for cin in (16, 32, 64) for cout in (16, 32, 64, 128) for (k, s) in GEOMS]


@pytest.mark.parametrize("case", CASES, ids=["c%d_%d_k%d_s%d" % c for c in CASES])
def test_f32act_layer(case):
    cin, cout, k, stride = case
    idx = CASES.index(case)
    N, H, W = SHAPES[idx % len(SHAPES)]
    rng, op, x, inv, shift = _case(idx, N, H, W, cin, cout, k, stride)
    want_name = "mfma_f32_act_c%d%s" % (cin, "_pw" if k == 1 else "_s2" if stride == 2 else "")
    Ho, Wo = -(-H // stride), -(-W // stride)
    res = leaky(rng.standard_normal((N, Ho, Wo, cout)).astype(F32))
    # (fn, act_bits, pool, shortcut, post_scale); the clips with a float32 output take this kernel too
    qb = (2, 4, 8)[idx % 3]
    variants = [(_abi.FN_LEAKY_RELU, 0, 1, None, 1.0), (_abi.FN_NONE, 0, 1, None, 1.0),
                (_abi.FN_LEAKY_RELU, 0, 1, res, 0.5), (_abi.FN_NONE, 0, 1, res, 1.0),
                (_abi.FN_BINARY_TANH, 0, 1, res, 0.5), (_abi.FN_QUANTIZED_TANH, qb, 1, None, 1.0)]
    if Ho >= 2 and Wo >= 2:
        variants += [(_abi.FN_LEAKY_RELU, 0, 2, None, 1.0), (_abi.FN_NONE, 0, 2, None, 1.0),
                     (_abi.FN_BINARY_TANH, 0, 2, None, 1.0), (_abi.FN_QUANTIZED_TANH, qb, 2, None, 1.0)]
    for fn, ab, pool, r, post in variants:
        msg = "fn=%d act_bits=%d pool=%d res=%s" % (fn, ab, pool, r is not None)
        got, kern = _run(op, x, inv, shift, fn, pool, r, post, ab)
        assert kern == want_name, (kern, want_name, msg)
        with valu_only():
            ref, rkern = _run(op, x, inv, shift, fn, pool, r, post, ab)
        assert rkern == "generic", msg
        np.testing.assert_array_equal(bits(got), bits(ref), err_msg=msg)
        want = _oracle(x, op, inv, shift, r, post, fn, pool, ab)
        np.testing.assert_array_equal(bits(got), bits(want), err_msg="oracle " + msg)


@pytest.mark.parametrize("wkind", range(len(WKINDS)), ids=["%s%s" % (k, n or "") for k, n in WKINDS])
def test_f32act_weight_kinds_batch64(wkind):
    """Every weight kind at N = 64, 3x3 64 -> 64 with BN, LeakyReLU and the 2x2 pool (the float VGG block)."""
    rng, op, x, inv, shift = _case(wkind * 6 + 3, 64, 8, 8, 64, 64, 3, 1)
    for fn, pool in ((_abi.FN_LEAKY_RELU, 2), (_abi.FN_LEAKY_RELU, 1)):
        got, kern = _run(op, x, inv, shift, fn, pool)
        assert kern == "mfma_f32_act_c64"
        with valu_only():
            ref, _ = _run(op, x, inv, shift, fn, pool)
        np.testing.assert_array_equal(bits(got), bits(ref))
        np.testing.assert_array_equal(bits(got), bits(_oracle(x, op, inv, shift, None, 1.0, fn, pool)))


# tests/test_gpu_parity.py FLOAT_CASES (input shape, cout, stride) with the kernel each takes under the default dispatch
# and under qnn_set_conv_impl(1); none of them has 16, 32 or 64 channels
FLOAT_CASES = [((3, 32, 32, 3), 64, 1, "mfma_f32_first_cin3", "ps_f32_cw3_k3"),
               ((2, 28, 28, 1), 64, 1, "mfma_f32_first_cin1", "ps_f32_cw1_k3"),
               ((2, 17, 13, 3), 16, 1, "ps_f32_cw3_k3", "ps_f32_cw3_k3"),
               ((2, 9, 9, 5), 6, 2, "generic", "generic"),
               ((2, 12, 10, 3), 256, 1, "mfma_f32_first_cin3", "ps_f32_cw3_k3"),
               ((2, 8, 8, 3), 128, 1, "mfma_f32_first_cin3", "ps_f32_cw3_k3")]


@pytest.mark.parametrize("case", FLOAT_CASES, ids=["%dx%dx%d_%d" % (c[0][1], c[0][2], c[0][3], c[1]) for c in FLOAT_CASES])
@pytest.mark.parametrize("pool", [1, 2])
def test_first_layer_shapes_keep_their_kernels(case, pool):
    """The float-input shapes with 1, 3 or 5 channels keep their kernels (exact names, both dispatch modes)."""
    xs, cout, stride, name_auto, name_valu = case
    rng = np.random.default_rng(1)
    x = (rng.integers(0, 256, xs).astype(F32) / F32(255)).astype(F32)
    op = {"op": "conv", "kind": "quantized", "nb": 4, "kernel": rng.uniform(-1, 1, (3, 3, xs[3], cout)).astype(F32),
          "bias": None, "strides": (stride, stride), "padding": "same"}
    got, kern = _run(op, x, None, None, _abi.FN_NONE, pool)
    assert kern == name_auto, kern
    with valu_only():
        ref, kern = _run(op, x, None, None, _abi.FN_NONE, pool)
    assert kern == name_valu, kern
    np.testing.assert_array_equal(bits(got), bits(ref))


def test_f32in_entry_leaky_relu():
    """qnn_conv2d_forward_f32in (binarize on load, BIN weights, 64 channels: the fused XNOR kernel's shape) with
    FN_LEAKY_RELU: that kernel does not implement it, so the call takes the packed route to k_conv_generic."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 8, 8, 64)).astype(F32)
    op = {"op": "conv", "kind": "binary", "kernel": rng.uniform(-1, 1, (3, 3, 64, 64)).astype(F32),
          "bias": (rng.standard_normal(64) * 0.5).astype(F32), "strides": (1, 1), "padding": "same"}
    w = engine._prepack(op, _abi.STORE_BIN, torch.device("cuda"))
    y, _, _ = _abi.conv2d_f32in(w, dev(x), _abi.FN_BINARY_TANH, 1, fn=_abi.FN_LEAKY_RELU)
    assert _abi.last_kernel() == "generic"
    want = _oracle(O.binary_tanh(x), op, None, None, None, 1.0, _abi.FN_LEAKY_RELU, 1)
    assert (want < 0).any()
    np.testing.assert_array_equal(bits(host(y)), bits(want))
    y, _, _ = _abi.conv2d_f32in(w, dev(x), _abi.FN_BINARY_TANH, 1)            # fn NONE keeps the fused kernel
    assert _abi.last_kernel().startswith("xnor_f32")
    np.testing.assert_array_equal(bits(host(y)), bits(_oracle(O.binary_tanh(x), op, None, None, None, 1.0, 0, 1)))


def test_leaky_relu_declined_by_other_kernels():
    """A 3-channel float input (the image) with FN_LEAKY_RELU: no first-layer kernel implements it -> generic."""
    rng = np.random.default_rng(2)
    x = leaky(rng.standard_normal((2, 12, 12, 3)).astype(F32))
    op = {"op": "conv", "kind": "binary", "kernel": rng.uniform(-1, 1, (3, 3, 3, 64)).astype(F32), "bias": None,
          "strides": (1, 1), "padding": "same"}
    got, kern = _run(op, x, None, None, _abi.FN_LEAKY_RELU, 1)
    assert kern == "generic"
    np.testing.assert_array_equal(bits(got), bits(_oracle(x, op, None, None, None, 1.0, _abi.FN_LEAKY_RELU, 1)))


# ---- networks -------------------------------------------------------------------------------------------------------
CODES = {"bf": (None, None), "tf": (None, None), "4f": (4, 4), "tt": (None, None)}


def _net(code):
    if code == "ff":    # float Conv2D x LeakyReLU: the float ResNet-20 of nets.build_spec
        return nets.build_spec(nets.Config(network_type="float", architecture="RESNET", nres=3, dim=32), 31)
    wb, ab = CODES[code]
    return nets.spec_from_keras_npz(os.path.join(GOLD, "resnet3_full_%s.npz" % code), wb, ab)


@pytest.mark.parametrize("code", ["bf", "tf", "4f", "ff", "tt"])
def test_resnet_checkpoint_fused(code, monkeypatch):
    spec = _net(code)
    x = nets.synthetic_images(nets.Config(dim=32), 6, 3)
    m = engine.ResidualFusedModel(spec[:-1], first_layer="exact")
    m.kernel_log = []
    where = []                                   # the separate LeakyReLU of the engine is a torch.where
    real_where = torch.where
    monkeypatch.setattr(torch, "where", lambda *a, **k: where.append(1) or real_where(*a, **k))
    got = host(m(dev(x)))
    monkeypatch.undo()
    with valu_only():
        ref = host(engine.ResidualFusedModel(spec[:-1], first_layer="exact")(dev(x)))
    np.testing.assert_array_equal(bits(got), bits(ref))
    want = O.run_spec(spec, x, float_conv="device")
    soft = host(_abi.softmax(dev(got)))
    np.testing.assert_allclose(soft, want, atol=2e-5)
    if code != "tt":
        nconv = sum(op["op"] == "conv" for op in spec)
        assert "generic" not in m.kernel_log, m.kernel_log
        assert len(m.kernel_log) == nconv, m.kernel_log                   # one launch per conv ...
        assert len(where) == 1, len(where)                                 # ... LeakyReLU fused after the first layer
        assert all(k.startswith("mfma_f32_act") for k in m.kernel_log[1:]), m.kernel_log


@pytest.mark.parametrize("code", ["bf", "tf"])
def test_predict_graph_matches_eager(code):
    spec = _net(code)
    cf = nets.Config(network_type="full-qnn", architecture="RESNET", nres=3, dim=32)
    x = nets.synthetic_images(cf, 2 * 4096 + 37, 9)
    model = nets.Model(cf, spec)
    got = model.predict(x)
    eager = np.concatenate([host(model.engine(dev(x[i:i + 4096]))) for i in range(0, len(x), 4096)])
    np.testing.assert_array_equal(bits(got), bits(eager))


def test_bnn_vgg_float_activations():
    """A bnn VGG (binary weights, LeakyReLU activations): its 64 -> 64 layers on the new kernel, bit-identical to VALU."""
    cf = nets.Config(network_type="bnn", architecture="VGG", dim=32)
    spec = nets.build_spec(cf, 5)
    x = nets.synthetic_images(cf, 5, 5)
    m = nets.Model(cf, spec, first_layer="exact").engine
    m.kernel_log = []
    got = host(m(dev(x)))
    assert any(k == "mfma_f32_act_c64" for k in m.kernel_log), m.kernel_log
    with valu_only():
        m2 = nets.Model(cf, spec, first_layer="exact").engine
        ref = host(m2(dev(x)))
    np.testing.assert_array_equal(bits(got), bits(ref))
