"""The int8 row-walking strip kernels (csrc/qnn_mfma_strip_i8.hip): 3x3 layers whose activations and weights are stored
as bytes, 16 / 32 / 64 input channels, stride 1 (with the residual merge) and stride 2.

Everything here is an integer / grid-valued path: every comparison is bit for bit, against the CPU oracle and against
the VALU kernel (k_conv_ps) on the same inputs.
"""
import os

import numpy as np
import pytest
import torch

import qnn_amd  # noqa: F401
from qnn_amd import _abi, engine, nets
from oracle import qnn_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BIN_ACT = {"op": "act", "fn": "binary_tanh"}
RING = 6            # row slots of the kernels' operand ring (QNN_STRIP8_SLOTS); small launches walk chunks of 4 rows


def Q(nb):
    return {"op": "act", "fn": "quantized_tanh", "nb": nb}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _rand_bn(rng, n, var):
    """Both signs of gamma."""
    return dict(op="bn", eps=1e-4, gamma=rng.uniform(-1.5, 1.5, n).astype(F32),
                beta=(rng.standard_normal(n) * 0.5).astype(F32),
                mean=(rng.standard_normal(n) * 0.1 * np.sqrt(var)).astype(F32),
                var=(var * rng.uniform(0.8, 1.25, n)).astype(F32))


def _conv_op(rng, cin, cout, stride=1, kind="quantized", nb=8, bias=True, kernel=None):
    op = {"op": "conv", "kind": kind, "kernel": rng.uniform(-1, 1, (3, 3, cin, cout)).astype(F32) if kernel is None else kernel,
          "bias": (rng.standard_normal(cout) * 0.05).astype(F32) if bias else None, "strides": (stride, stride),
          "padding": "same"}
    if kind == "quantized":
        op["nb"] = nb
    return op


def _oracle(x, op, bn, act, short=None, pool=1):
    """conv -> bn [-> (shortcut + y) * 0.5] -> act [-> maxpool] as the oracle computes the ops one by one."""
    t = O.run_spec([dict(op)] + ([bn] if bn is not None else []), x)
    if short is not None:
        t = ((short + t).astype(F32) * F32(0.5)).astype(F32)          # models/resnet.py:127-128
    tail = ([act] if act is not None else []) + ([{"op": "maxpool", "size": 2}] if pool == 2 else [])
    return O.run_spec(tail, t) if tail else t


def _launch(x, x_bits, op, bn, act, short=None, short_bits=None, out_store=_abi.STORE_I8, pool=1, trick=None):
    """One qnn_conv2d_forward call with int8-stored operands.  x: values on the x_bits grid; short: None, float32 values
    (short_bits None: the float32 shortcut) or values on the short_bits grid (packed int8 shortcut).
    Returns (output values, kernel name)."""
    N, H, W, C = x.shape
    st = op["strides"][0]
    cout = op["kernel"].shape[3]
    xin = _abi.pack(dev(x), C, _abi.FN_GRID, x_bits, _abi.STORE_I8)
    w = engine._prepack(op, _abi.STORE_I8, torch.device("cuda"), stride=st, same_pad=True)
    inv = shift = None
    if bn is not None:
        i, s = engine.bn_constants(bn)
        inv, shift = dev(i), dev(s)
    fn, abits = engine._act_code(act) if act is not None else (_abi.FN_NONE, 0)
    rkw = {}
    if short is not None and short_bits is None:
        rkw = dict(res=dev(short), res_store=_abi.STORE_F32, res_bits=0, post_scale=0.5)
    elif short is not None:
        rkw = dict(res=_abi.pack(dev(short), cout, _abi.FN_GRID, short_bits, _abi.STORE_I8), res_store=_abi.STORE_I8,
                   res_bits=short_bits, post_scale=0.5)
    y, Ho, Wo = _abi.conv2d(w, xin, _abi.STORE_I8, x_bits, N, H, W, inv, shift, fn,
                            abits if fn == _abi.FN_QUANTIZED_TANH else 0, pool, out_store, trick=trick, **rkw)
    kern = _abi.last_kernel()
    if out_store == _abi.STORE_F32:
        return host(y), kern
    return host(_abi.unpack(y, N * Ho * Wo, cout, out_store, abits if abits else 1)).reshape(N, Ho, Wo, cout), kern


def _name(cin, stride):
    return "strip_i8_c%d%s" % (cin, "_s2" if stride == 2 else "")


def _check(x, x_bits, op, bn, act, short=None, short_bits=None):
    """The strip kernel against the oracle and against the VALU kernel on the same inputs."""
    cin, st = x.shape[3], op["strides"][0]
    got, kern = _launch(x, x_bits, op, bn, act, short, short_bits)
    assert kern == _name(cin, st), kern
    np.testing.assert_array_equal(got, _oracle(x, op, bn, act, short))
    _abi.set_conv_impl(_abi.IMPL_VALU)
    try:
        valu, kv = _launch(x, x_bits, op, bn, act, short, short_bits)
    finally:
        _abi.set_conv_impl(_abi.IMPL_AUTO)
    assert not kv.startswith("strip"), kv
    np.testing.assert_array_equal(got, valu)


# the five forms: (cin, cout, stride)
FORMS = [(16, 16, 1), (32, 32, 1), (64, 64, 1), (16, 32, 2), (32, 64, 2)]


@pytest.mark.parametrize("cin,cout,stride", FORMS, ids=[_name(c, s) for c, _, s in FORMS])
def test_dispatch(cin, cout, stride):
    """Auto mode takes the strip form; the VALU preference, QNN_EPI_NO_STRIP, a pooled layer, a float32 output and the
    faithful trick keep the kernels these calls had before."""
    rng = np.random.default_rng(cin + stride)
    x = O.run_spec([Q(8)], rng.standard_normal((2, 6, 20, cin)).astype(F32))
    op = _conv_op(rng, cin, cout, stride)
    bn = _rand_bn(rng, cout, 9 * cin * 0.12)
    old = "mfma_i8_areg64x64" if cin == 64 else "ps_i8_cw%d_k3" % (cin // 4)
    got, kern = _launch(x, 8, op, bn, Q(8))
    assert kern == _name(cin, stride), kern
    want = _oracle(x, op, bn, Q(8))
    np.testing.assert_array_equal(got, want)
    _abi.set_conv_impl(_abi.IMPL_VALU)
    try:
        got, kern = _launch(x, 8, op, bn, Q(8))
        assert kern == "ps_i8_cw%d_k3" % (cin // 4), kern
        np.testing.assert_array_equal(got, want)
    finally:
        _abi.set_conv_impl(_abi.IMPL_AUTO)
    _abi.set_option("strip", 0)
    try:
        got, kern = _launch(x, 8, op, bn, Q(8))
        assert kern == old, kern
        np.testing.assert_array_equal(got, want)
    finally:
        _abi.set_option("strip", 1)
    if cin == 64:                                  # the A/B switch of the 64-channel layers
        _abi.set_option("strip64", 0)
        try:
            got, kern = _launch(x, 8, op, bn, Q(8))
            assert kern == old, kern
            np.testing.assert_array_equal(got, want)
        finally:
            _abi.set_option("strip64", -1)
    got, kern = _launch(x, 8, op, bn, Q(8), pool=2)
    assert kern == old, kern
    np.testing.assert_array_equal(got, _oracle(x, op, bn, Q(8), pool=2))
    got, kern = _launch(x, 8, op, bn, Q(8), out_store=_abi.STORE_F32)
    assert kern == old, kern
    np.testing.assert_array_equal(got, want)
    got, kern = _launch(x, 8, op, bn, Q(4), out_store=_abi.STORE_I4)       # int4 output from int8 inputs
    assert not kern.startswith("strip"), kern
    np.testing.assert_array_equal(got, _oracle(x, op, bn, Q(4)))
    _, kern = _launch(x, 8, op, bn, Q(8), trick=_abi.faithful_trick(F32(1.0) / F32(np.sqrt(1.5 / (9 * cin + 9 * cout)))))
    assert kern == "ps_i8_cw%d_k3" % (cin // 4), kern


GEOMETRY = [
    # cin, cout, stride, N, H, W
    (16, 16, 1, 1, 1, 16), (16, 16, 1, 3, 2, 24), (16, 16, 1, 1, 3, 37), (16, 16, 1, 3, 7, 16), (16, 16, 1, 1, RING - 1, 218),
    (16, 16, 1, 3, RING + 1, 24), (16, 16, 1, 260, 5, 16), (16, 16, 1, 260, 7, 218), (16, 48, 1, 3, 9, 37),
    (32, 32, 1, 1, 1, 37), (32, 32, 1, 3, 2, 16), (32, 32, 1, 3, 3, 24), (32, 32, 1, 1, 7, 218), (32, 32, 1, 260, RING - 1, 24),
    (32, 32, 1, 3, RING + 1, 37), (32, 32, 1, 1, 13, 16), (32, 96, 1, 3, 5, 24),
    (64, 64, 1, 1, 1, 24), (64, 64, 1, 3, 2, 37), (64, 64, 1, 1, 3, 16), (64, 64, 1, 3, 7, 24), (64, 64, 1, 1, RING - 1, 218),
    (64, 64, 1, 260, RING + 1, 16), (64, 64, 1, 3, 9, 37),
    (16, 32, 2, 1, 1, 16), (16, 32, 2, 3, 2, 37), (16, 32, 2, 3, 3, 24), (16, 32, 2, 1, 7, 218), (16, 32, 2, 260, 9, 16),
    (16, 32, 2, 3, 2 * RING + 1, 37), (16, 32, 2, 1, 10, 24),
    (32, 64, 2, 1, 1, 24), (32, 64, 2, 3, 2, 16), (32, 64, 2, 1, 3, 37), (32, 64, 2, 3, 7, 218), (32, 64, 2, 260, 10, 24),
    (32, 64, 2, 3, 2 * RING - 1, 16), (32, 64, 2, 1, 9, 37),
]


@pytest.mark.parametrize("cin,cout,stride,N,H,W", GEOMETRY, ids=["%d_%d_s%d_n%d_%dx%d" % g for g in GEOMETRY])
def test_geometry(cin, cout, stride, N, H, W):
    """Widths that are and are not multiples of 16, heights around the ring depth and the row chunk, one to 260 images;
    with and without a bias; every shortcut form of the stride-1 kernels."""
    rng = np.random.default_rng(cin * 7 + cout + 1000 * stride + H * 31 + W + N)
    x = O.run_spec([Q(8)], rng.standard_normal((N, H, W, cin)).astype(F32))
    bn = _rand_bn(rng, cout, 9 * cin * 0.12)
    bias = (H + W) % 2 == 0
    op = _conv_op(rng, cin, cout, stride, bias=bias)
    _check(x, 8, op, bn, Q(8))
    if N > 100:
        return
    _check(x, 8, _conv_op(rng, cin, cout, stride, bias=not bias), bn, Q(8))
    if stride == 1:
        sf = rng.standard_normal((N, H, W, cout)).astype(F32)
        _check(x, 8, op, bn, Q(8), short=O.run_spec([Q(8)], sf), short_bits=8)
        _check(x, 8, op, bn, Q(8), short=O.run_spec([Q(4)], sf), short_bits=4)
        _check(x, 8, op, bn, Q(8), short=(sf * F32(0.37)).astype(F32))                 # float32 shortcut (projection blocks)


@pytest.mark.parametrize("cin,cout,stride", FORMS, ids=[_name(c, s) for c, _, s in FORMS])
@pytest.mark.parametrize("wkind,wnb", [("quantized", 2), ("quantized", 4), ("quantized", 8), ("binary", None), ("ternary", None)])
def test_number_formats(cin, cout, stride, wkind, wnb):
    """Activation codes of 4 and 8 bits held in bytes, output codes of 2 / 4 / 5 / 8 bits and +-1 into bytes, weights of
    2 / 4 / 8 bits and binary / ternary weights held in bytes; shortcut codes of 4 and 8 bits."""
    rng = np.random.default_rng(cin + 3 * stride + (wnb or 0) + len(wkind))
    H, W, N = 7, 24, 2
    op = _conv_op(rng, cin, cout, stride, kind=wkind, nb=wnb)
    wvar = {2: 0.4, 4: 0.33, 8: 0.33}.get(wnb, 1.0 if wkind == "binary" else 0.5)
    for x_bits in (4, 8):
        x = O.run_spec([Q(x_bits)], rng.standard_normal((N, H, W, cin)).astype(F32))
        bn = _rand_bn(rng, cout, 9 * cin * 0.4 * wvar)
        for act in (Q(2), Q(4), Q(5), Q(8), BIN_ACT):
            _check(x, x_bits, op, bn, act)
        if stride == 1:
            sf = rng.standard_normal((N, H, W, cout)).astype(F32)
            _check(x, x_bits, op, bn, Q(x_bits), short=O.run_spec([Q(x_bits)], sf), short_bits=x_bits)
            _check(x, x_bits, op, bn, Q(5), short=O.run_spec([Q(8)], sf), short_bits=8)


@pytest.mark.parametrize("cin,cout,stride", FORMS, ids=[_name(c, s) for c, _, s in FORMS])
@pytest.mark.parametrize("xfill,wfill", [(1.0, 1.0), (-1.0, -1.0), (-1.0, 1.0), (1.0, -1.0)])
def test_saturated(cin, cout, stride, xfill, wfill):
    """All-max / all-min codes against all-max / all-min weights: the largest accumulators of these layers, 9 * Cin *
    (128 * 128 or 127 * 127 or -128 * 127) -- 9 437 184 in magnitude at Cin 64, below 2^24."""
    rng = np.random.default_rng(5)
    H, W, N = 5, 20, 2
    x = O.run_spec([Q(8)], np.full((N, H, W, cin), xfill, F32))
    op = _conv_op(rng, cin, cout, stride, bias=False, kernel=np.full((3, 3, cin, cout), wfill, F32))
    plain = O.run_spec([dict(op)], x)
    full = float(np.abs(plain).max())
    assert full >= 9 * cin * (127.0 / 128) ** 2                # the interior pixels see all 9 * Cin products
    # BN centred between the border and the interior sums, so that the 8-bit codes do not all clip
    sign = 1.0 if xfill * wfill > 0 else -1.0
    bn = dict(op="bn", eps=1e-4, gamma=rng.uniform(-1.5, 1.5, cout).astype(F32), beta=(rng.standard_normal(cout) * 0.2).astype(F32),
              mean=np.full(cout, sign * 0.7 * full, F32), var=np.full(cout, (0.4 * full) ** 2, F32))
    _check(x, 8, op, bn, Q(8))
    if stride == 1:
        short = O.run_spec([Q(8)], np.full((N, H, W, cout), xfill, F32))
        _check(x, 8, op, bn, Q(8), short=short, short_bits=8)
        # float32 shortcut cancelling all but 1 / 1024 of the raw sum
        _check(x, 8, op, None, Q(8), short=(-plain * F32(1.0 - 1.0 / 1024)).astype(F32))


def test_trained_48_kernel():
    """The 3x3 layer the `48` fixture holds (results/RESNET3/weights_48.hdf5: 8-bit weights, 4-bit activations kept in
    bytes; conv2 with its bias and bn2), plain and with the packed 4-bit shortcut of its block."""
    d = np.load(os.path.join(GOLD, "resnet3_48.npz"))
    rng = np.random.default_rng(48)
    op = {"op": "conv", "kind": "quantized", "nb": 8, "kernel": d["conv2_kernel"], "bias": d["conv2_bias"], "strides": (1, 1),
          "padding": "same"}
    bn = dict(op="bn", eps=1e-3, gamma=d["bn2_gamma"], beta=d["bn2_beta"], mean=d["bn2_moving_mean"], var=d["bn2_moving_variance"])
    x = O.run_spec([Q(4)], rng.standard_normal((5, 32, 32, 16)).astype(F32))
    _check(x, 4, op, bn, Q(4))
    short = O.run_spec([Q(4)], rng.standard_normal((5, 32, 32, 16)).astype(F32))
    _check(x, 4, op, bn, Q(4), short=short, short_bits=4)


def _small_convs(spec):
    """The 3x3 convolutions with 16 or 32 input channels."""
    return [op for op in spec if op["op"] == "conv" and op["kernel"].shape[0] == 3 and op["kernel"].shape[2] in (16, 32)]


def _check_log(log, spec):
    strips = [k for k in log if k.startswith(("strip_i8_c16", "strip_i8_c32"))]
    assert len(strips) == len(_small_convs(spec)), log
    assert not any(k.startswith("ps_i8") and k.endswith("_k3") for k in log), log
    assert "generic" not in log, log


@pytest.mark.parametrize("wb,ab", [(8, 8), (8, 4)])
def test_resnet20(wb, ab):
    """CIFAR ResNet-20 (nres = 3), 8-bit weights with 8- and 4-bit activations: logits bit for bit through the residual
    engine (exact first layer; bytes / 255 through the "auto" first layer) and through hipGraph replay on two lanes."""
    cf = nets.Config(network_type="full-qnn", wbits=wb, abits=ab, architecture="RESNET", nres=3, dim=32)
    spec = nets.resnet_spec(cf, 20 + ab)[:-1]
    assert len(_small_convs(spec)) == 13
    x = nets.synthetic_images(cf, 3, 7)
    want = O.run_spec(spec, x, float_conv="device")
    m = engine.ResidualFusedModel(spec, first_layer="exact")
    m.kernel_log = []
    np.testing.assert_array_equal(host(m(dev(x))), want)
    _check_log(m.kernel_log, spec)
    # the merges are inside the conv launches: one launch per convolution
    assert len(m.kernel_log) == sum(op["op"] == "conv" for op in spec), m.kernel_log
    gm = engine.GraphModel(spec)
    np.testing.assert_array_equal(host(gm(dev(x))), want)
    xu8 = nets.synthetic_images_u8(cf, 6, 9)
    xb = (xu8.astype(F32) / F32(255)).astype(F32)
    want8 = O.run_spec_u8(spec, xu8)
    ma = engine.ResidualFusedModel(spec, first_layer="auto")
    ma.kernel_log = []
    np.testing.assert_array_equal(host(ma(dev(xb))), want8)
    _check_log(ma.kernel_log, spec)
    pipe = engine.Pipelined(ma, lanes=2, batch_size=2)
    np.testing.assert_array_equal(host(pipe(dev(xb))), want8)
    pipe.check_domain()
    pipe3 = engine.Pipelined(m, lanes=3, batch_size=1)
    np.testing.assert_array_equal(host(pipe3(dev(x))), want)


def test_imagenet224_resnet10_w8a8():
    """The ImageNet-224 geometry (224 / 112 / 56 wide stages, nres = 10: 41 of the 63 convolutions have 16 or 32 input
    channels): one image against the oracle, and batch independence at 64 images."""
    base = nets.baseline_config(4)
    cf = nets.Config(network_type="full-qnn", wbits=8, abits=8, architecture="RESNET", nres=10, dim=224,
                     channels=base.channels, classes=base.classes)
    spec = nets.resnet_spec(cf, 224)[:-1]
    assert sum(op["op"] == "conv" for op in spec) == 63 and len(_small_convs(spec)) == 41
    x = nets.synthetic_images(cf, 64, 5)
    want = O.run_spec(spec, x[:1], float_conv="device")
    m = engine.ResidualFusedModel(spec, first_layer="exact")
    m.kernel_log = []
    one = host(m(dev(x[:1])))
    np.testing.assert_array_equal(one, want)
    _check_log(m.kernel_log, spec)
    m.kernel_log = []
    batch = host(m(dev(x)))
    _check_log(m.kernel_log, spec)
    np.testing.assert_array_equal(batch[:1], one)
    again = host(m(dev(x[63:])))
    np.testing.assert_array_equal(batch[63:], again)
