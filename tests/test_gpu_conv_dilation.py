"""dilation_rate on the GPU: the generic kernel on every input store, the matrix-pipe strip kernel
(csrc/qnn_mfma_strip_dil.hip), the refusals, the Keras classes and the engines.

Expected values: the plain convolution with the zero-stuffed kernel through oracle.conv2d (proven against torch in
tests/test_conv_dilation_cpu.py).  All tensors are dyadic, so every comparison is bit for bit, without a tolerance.
Every launch asserts _abi.last_kernel()."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi, engine
from oracle import qnn_oracle as O
import conv_dilation_cases as D

pytestmark = pytest.mark.gpu
F32 = np.float32
CUDA = torch.device("cuda")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "quantizedneuralnetworks-keras-tensorflow_amd", "csrc")
STORE = {"f32": _abi.STORE_F32, "u8": _abi.STORE_U8, "bin": _abi.STORE_BIN, "t2": _abi.STORE_T2, "i4": _abi.STORE_I4,
         "i8": _abi.STORE_I8}
ABITS = {"f32": 0, "u8": 0, "bin": 1, "t2": 1, "i4": 4, "i8": 8}
Q4 = {"op": "act", "fn": "quantized_tanh", "nb": 4}
Q8 = {"op": "act", "fn": "quantized_tanh", "nb": 8}
BT = {"op": "act", "fn": "binary_tanh"}
# epilogue: (activation op or None, fn, act_bits, out_store)
EPI = {"f32": (None, _abi.FN_NONE, 0, _abi.STORE_F32), "q4_f32": (Q4, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_F32),
       "q4_i4": (Q4, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4), "q4_i8": (Q4, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I8),
       "q8_i8": (Q8, _abi.FN_QUANTIZED_TANH, 8, _abi.STORE_I8), "bin": (BT, _abi.FN_BINARY_TANH, 1, _abi.STORE_BIN),
       "bt_i4": (BT, _abi.FN_BINARY_TANH, 1, _abi.STORE_I4),
       "leaky": ({"op": "act", "fn": "leaky_relu", "alpha": 0.3}, _abi.FN_LEAKY_RELU, 0, _abi.STORE_F32)}
GENERIC_EPIS = {"f32": ("f32", "q4_i4"), "u8": ("f32", "q4_i4", "bin"), "bin": ("f32", "bin"), "t2": ("f32", "q4_i8"),
                "i4": ("q4_f32", "q4_i4"), "i8": ("f32", "q8_i8")}
IMPLS = (_abi.IMPL_VALU, _abi.IMPL_AUTO)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def bn_pow2(K, cout):
    """Per-channel scale +-2^-j (odd channels negative) and a dyadic shift."""
    j = max(0, int(np.ceil(np.log2(np.sqrt(K)))) - 1)
    inv = np.where(np.arange(cout) % 2 == 0, 1.0, -1.0) * 2.0 ** -j
    return inv.astype(F32), (((np.arange(cout) % 5) - 2) / 16.0).astype(F32)


def unpacked(y, n, hp, wp, cout, out_store, ab):
    if out_store == _abi.STORE_F32:
        return host(y)
    return host(_abi.unpack(y, n * hp * wp, cout, out_store, ab)).reshape(n, hp, wp, cout)


def expected(kind, x, k, bias, g, inv, shift, act, res=None, pool=1):
    """The layer through the oracle on the zero-stuffed kernel: conv + bias, BN, [(res + v) / 2], activation, [pool]."""
    ks = D.stuff(k, g["dh"], g["dw"])
    if kind == "u8":
        op = D.conv_op(kind, g, ks, bias)
        del op["dilation_rate"]
        want = O.u8_conv_group(x, op, None, act)
    else:
        want = (O.conv2d(x, ks, (1, 1), g["padding"]) + bias).astype(F32)
        want = (want * inv + shift).astype(F32)
        if res is not None:
            want = ((res + want).astype(F32) * F32(0.5)).astype(F32)
        if act is not None:
            want = O.run_spec([act], want)
    return O.maxpool2d(want, pool) if pool == 2 else want


def run_generic(kind, g, cin, cout, epis, n=D.N, res=None, pool=1, values=None, salt=0):
    """One dilated layer on k_conv_generic under both kernel families against the oracle; an empty output is refused."""
    x, k, bias = values if values is not None else D.layer_values(kind, g, cin, cout, n, salt)
    inv, shift = bn_pow2(g["kh"] * g["kw"] * cin, cout)
    use_bn = kind != "u8"                        # the byte entry has its own affine form: bias only here
    store = STORE[kind]
    wstore = _abi.STORE_F32 if kind in ("f32", "u8") else store
    xd = dev(x) if kind in ("f32", "u8") else _abi.pack(dev(x), cin, _abi.FN_GRID, ABITS[kind], store)
    w = engine._prepack(D.conv_op(kind, g, k, bias), wstore, CUDA, stride=1, same_pad=g["padding"] == "same")
    assert w.dilation == (g["dh"], g["dw"])
    Ho, Wo = D.out_hw(g)
    if Ho // pool <= 0 or Wo // pool <= 0:
        with pytest.raises(_abi.QnnError, match="empty output"):
            _abi.conv2d(w, xd, store, ABITS[kind], n, g["H"], g["W"], pool=pool)
        return
    rkw, res_val = {}, None
    if res is not None:
        rng = np.random.default_rng(D.seed_of(g, salt) + 5)
        res_val = (D.codes(rng, (n, Ho, Wo, cout), -8, 7) / 8.0).astype(F32)
        rkw = dict(res=dev(res_val), res_store=_abi.STORE_F32, res_bits=0, post_scale=0.5) if res == "f32" else \
            dict(res=_abi.pack(dev(res_val), cout, _abi.FN_GRID, 4, _abi.STORE_I4), res_store=_abi.STORE_I4, res_bits=4,
                 post_scale=0.5)
    try:
        for epi in epis:
            act, fn, ab, out_store = EPI[epi]
            want = expected(kind, x, k, bias, g, inv, shift, act, res_val, pool)
            assert want.shape == (n, Ho // pool, Wo // pool, cout)
            for impl in IMPLS:
                _abi.set_conv_impl(impl)
                y, hp, wp = _abi.conv2d(w, xd, store, ABITS[kind], n, g["H"], g["W"], dev(inv) if use_bn else None,
                                        dev(shift) if use_bn else None, fn, ab, pool, out_store, **rkw)
                name = _abi.last_kernel()
                what = "%s %s cin=%d cout=%d %s impl=%d kernel=%s" % (kind, D.geom_id(g), cin, cout, epi, impl, name)
                assert (hp, wp) == (Ho // pool, Wo // pool), what
                np.testing.assert_array_equal(unpacked(y, n, hp, wp, cout, out_store, ab), want, err_msg=what)
                assert name == ("generic_u8" if kind == "u8" else "generic"), what
    finally:
        _abi.set_conv_impl(_abi.IMPL_AUTO)


# ---- the generic kernel, every input store ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(D.GENERIC))
@pytest.mark.parametrize("window", D.WINDOWS, ids=lambda w: "%dx%d" % w)
def test_generic_kernel_on_the_whole_list(kind, window):
    cin, cout = D.GENERIC[kind]
    for g in (g for g in D.geometries() if (g["kh"], g["kw"]) == window):
        run_generic(kind, g, cin, cout, GENERIC_EPIS[kind])


def gm(kh, kw, dh, dw, padding, H, W):
    return dict(kh=kh, kw=kw, dh=dh, dw=dw, padding=padding, H=H, W=W)


def test_generic_kernel_pool_residual_and_the_other_activations():
    # a pooled case behind an odd conv map (7 x 9 -> 3 x 4), per store
    for kind in sorted(D.GENERIC):
        cin, cout = D.GENERIC[kind]
        run_generic(kind, gm(3, 3, 2, 2, "same", 7, 9), cin, cout, GENERIC_EPIS[kind], pool=2)
        run_generic(kind, gm(2, 3, 1, 2, "valid", 7, 9), cin, cout, GENERIC_EPIS[kind][-1:], pool=2)
    # float32 and packed residual, binary_tanh into int4 codes, LeakyReLU
    for kind, epi in (("i4", "q4_i4"), ("f32", "q4_f32"), ("bin", "bin"), ("i8", "q8_i8"), ("t2", "q4_i8")):
        cin, cout = D.GENERIC[kind]
        run_generic(kind, gm(3, 3, 2, 3, "same", 7, 9), cin, cout, (epi,), res="packed")
        run_generic(kind, gm(3, 1, 3, 1, "valid", 7, 9), cin, cout, (epi,), res="f32")
    run_generic("i4", gm(3, 3, 2, 2, "same", 7, 9), 24, 10, ("bt_i4",))
    run_generic("f32", gm(3, 3, 5, 5, "same", 7, 9), 5, 10, ("leaky",))
    run_generic("i4", gm(3, 3, 8, 1, "same", 7, 9), 24, 10, ("q4_i4",))          # the two axes are independent, up to 8
    run_generic("i4", gm(3, 3, 1, 8, "same", 7, 9), 24, 10, ("q4_i4",))


@pytest.mark.parametrize("sign_x,sign_w", [(1, 1), (1, -1), (-1, 1), (-1, -1)])
def test_binary_same_padding_with_a_dilated_border(sign_x, sign_w):
    """BIN + SAME: the border of a dilated window is d pixels deep.  With constant inputs and weights every output is
    +-cin times the number of taps INSIDE the image, so a padded tap counted as -1 (or a correction built for a one-pixel
    border) shows in every border class: 5x5 with d = 2 and 3x3 with d = 3 (only the centre tap is ever inside)."""
    cin, cout = 24, 10
    for size, d in ((5, 2), (3, 3)):
        g = gm(3, 3, d, d, "same", size, size)
        x = np.full((D.N, size, size, cin), sign_x, F32)
        k = np.full((3, 3, cin, cout), sign_w, F32)
        inside = np.array([sum(0 <= c + t * d < size for t in (-1, 0, 1)) for c in range(size)])
        taps = inside[:, None] * inside[None, :]
        if size == 3:
            assert (taps == 1).all()
        _abi.set_conv_impl(_abi.IMPL_AUTO)
        w = engine._prepack(D.conv_op("bin", g, k, None), _abi.STORE_BIN, CUDA, stride=1, same_pad=True)
        y, _, _ = _abi.conv2d(w, _abi.pack(dev(x), cin, _abi.FN_GRID, 1, _abi.STORE_BIN), _abi.STORE_BIN, 1, D.N, size, size)
        assert _abi.last_kernel() == "generic"
        want = np.broadcast_to((sign_x * sign_w * cin * taps).astype(F32)[None, :, :, None], (D.N, size, size, cout))
        np.testing.assert_array_equal(host(y), want)
        run_generic("bin", g, cin, cout, ("f32", "bin"), values=(x, k, np.zeros(cout, F32)))
    # random signs on the same two images, and with the clip fused on load (qnn_conv2d_forward_f32in)
    for size, d in ((5, 2), (3, 3)):
        g = gm(3, 3, d, d, "same", size, size)
        run_generic("bin", g, 33, 10, ("f32", "bin"), salt=2)
        x, k, bias = D.layer_values("bin", g, 64, 64, salt=3)
        w = engine._prepack(D.conv_op("bin", g, k, bias), _abi.STORE_BIN, CUDA, stride=1, same_pad=True)
        y, _, _ = _abi.conv2d_f32in(w, dev(x), _abi.FN_BINARY_TANH, 1)
        assert _abi.last_kernel() == "generic"
        np.testing.assert_array_equal(host(y), (O.conv2d(x, D.stuff(k, d, d)) + bias).astype(F32))


# ---- the strip kernel --------------------------------------------------------------------------------------------------
def strip_layer(cin, cout, d, n, H, W, salt=0):
    g = gm(3, 3, d, d, "same", H, W)
    x, k, bias = D.layer_values("i4", g, cin, cout, n, salt)
    return g, x, k, bias


def run_strip(cin, cout, d, shape, res, claimed, values=None, bias_on=True, epi="q4_i4"):
    """One 3x3 'same' int4 -> int4 layer: by default on strip_i4_c<cin>_dil where the route claims d, on the generic kernel
    under QNN_EPI_NO_STRIP and for an unclaimed d; the outputs equal each other and the oracle."""
    n, H, W = shape
    g = gm(3, 3, d, d, "same", H, W)
    x, k, bias = values if values is not None else D.layer_values("i4", g, cin, cout, n)
    if not bias_on:
        bias = None
    inv, shift = bn_pow2(9 * cin, cout)          # negative scales on the odd channels
    act, fn, ab, out_store = EPI[epi]
    rkw, res_val = {}, None
    if res is not None:
        rng = np.random.default_rng(D.seed_of(g) + 5)
        res_val = (D.codes(rng, (n, H, W, cout), -8, 7) / 8.0).astype(F32)
        rkw = dict(res=dev(res_val), res_store=_abi.STORE_F32, res_bits=0, post_scale=0.5) if res == "f32" else \
            dict(res=_abi.pack(dev(res_val), cout, _abi.FN_GRID, 4, _abi.STORE_I4), res_store=_abi.STORE_I4, res_bits=4,
                 post_scale=0.5)
    want = expected("i4", x, k, bias if bias is not None else F32(0), g, inv, shift, act, res_val)
    w = engine._prepack(D.conv_op("i4", g, k, bias), _abi.STORE_I4, CUDA, stride=1, same_pad=True)
    xd = _abi.pack(dev(x), cin, _abi.FN_GRID, 4, _abi.STORE_I4)
    outs = []
    try:
        for strip in (1, 0):
            _abi.set_option("strip", strip)
            y, hp, wp = _abi.conv2d(w, xd, _abi.STORE_I4, 4, n, H, W, dev(inv), dev(shift), fn, ab, 1, out_store, **rkw)
            name = _abi.last_kernel()
            what = "cin=%d cout=%d d=%d %s res=%s strip=%d kernel=%s" % (cin, cout, d, shape, res, strip, name)
            assert name == ("strip_i4_c%d_dil" % cin if strip and claimed else "generic"), what
            outs.append(host(y))
            np.testing.assert_array_equal(unpacked(y, n, hp, wp, cout, out_store, ab), want, err_msg=what)
    finally:
        _abi.set_option("strip", 1)
    np.testing.assert_array_equal(outs[0], outs[1])


@pytest.mark.parametrize("d", D.STRIP_CLAIMED + (D.STRIP_UNCLAIMED,))
@pytest.mark.parametrize("cin", D.STRIP_CIN)
def test_strip_kernel_equals_the_generic_kernel_and_the_oracle(cin, d):
    cmul = 16 if cin == 16 else 32
    claimed = d in D.STRIP_CLAIMED
    for i, shape in enumerate(D.STRIP_IMAGES):
        for j, cout in enumerate((cmul, 2 * cmul)):
            for m, res in enumerate((None, "packed", "f32")):
                if not claimed and (i + j + m) % 3:          # the unclaimed rate runs the generic kernel: a third of the grid
                    continue
                run_strip(cin, cout, d, shape, res, claimed, bias_on=(i + j + m) % 2 == 0)
    run_strip(cin, cmul, d, (3, 5, 16), "packed", claimed, epi="bt_i4")


@pytest.mark.parametrize("d", D.STRIP_CLAIMED)
@pytest.mark.parametrize("cin", D.STRIP_CIN)
def test_strip_kernel_reads_no_tap_across_an_image_boundary(cin, d):
    """Three images, the middle one all code 7, the outer ones all -8, all weights positive: a tap read from the
    neighbouring image instead of the zero padding changes a sum."""
    cout = 32
    x = np.full((3, 5, 16, cin), -1.0, F32)
    x[1] = 7 / 8.0
    k = np.full((3, 3, cin, cout), 1 / 8.0, F32)
    for res in (None, "packed"):
        run_strip(cin, cout, d, (3, 5, 16), res, True, values=(x, k, np.zeros(cout, F32)))


def test_strip_plan_cuts_the_tall_image(tmp_path):
    """Which of STRIP_IMAGES walk several row chunks per strip, from csrc/qnn_strip_plan.h compiled on its own with the
    kernel's arguments (Cin 16: blocks_cap 1024, fill 2d + 2 = 6; far fewer tasks than waves, so a round costs rc + fill
    and the shortest chunk, four rows, wins): every image above four rows.  5 is the smallest such height -- (3, 5, 16)
    is cut into 4 + 1 rows -- and (1, 40, 16) walks ten chunks, with the ring re-filled at every chunk start."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "plan_main.cpp"
    src.write_text('#include <stdio.h>\n#include "qnn_strip_plan.h"\nint main() { for (int H = 1; H <= 64; ++H) { StripPlan p; '
                   'if (!qnn_strip_plan(&p, 1, 1, H, 1024, 6, 1)) return 1; printf("%d %d\\n", H, p.nch); } return 0; }\n')
    subprocess.run([cxx, "-std=c++17", "-I", CSRC, str(src), "-o", str(tmp_path / "plan_main")], check=True)
    out = subprocess.run([str(tmp_path / "plan_main")], check=True, capture_output=True, text=True).stdout.split()
    nch = dict(zip(map(int, out[0::2]), map(int, out[1::2])))
    assert [h for h in sorted(nch) if nch[h] > 1][0] == 5 and nch[D.TALL[1]] == 10
    assert D.TALL in D.STRIP_IMAGES and (3, 5, 16) in D.STRIP_IMAGES


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    g = gm(3, 3, 2, 2, "same", 8, 8)
    x, k, bias = D.layer_values("i4", g, 64, 64)
    op = D.conv_op("i4", g, k, bias)
    with pytest.raises(_abi.QnnError, match="together with stride 2"):
        engine._prepack(op, _abi.STORE_I4, CUDA, stride=2, same_pad=True)
    with pytest.raises(_abi.QnnError, match="must be >= 1"):
        engine._prepack(dict(op, dilation_rate=(0, 1)), _abi.STORE_I4, CUDA)
    w = engine._prepack(op, _abi.STORE_I4, CUDA)
    xd = _abi.pack(dev(x), 64, _abi.FN_GRID, 4, _abi.STORE_I4)
    inv, shift = (dev(a) for a in bn_pow2(9 * 64, 64))
    y, _, _ = _abi.conv2d(w, xd, _abi.STORE_I4, 4, D.N, 8, 8, inv, shift, _abi.FN_QUANTIZED_TANH, 4, 1, _abi.STORE_I4)
    assert _abi.last_kernel() == "strip_i4_c64_dil"
    # the fused conv + classifier entry
    dk = (D.codes(np.random.default_rng(1), (1024, 10), -8, 7) / 8.0).astype(F32)
    wd = engine._prepack({"op": "dense", "kind": "quantized", "nb": 4, "kernel": dk, "bias": None}, _abi.STORE_I4, CUDA)
    with pytest.raises(_abi.QnnError, match="dilated"):
        _abi.conv2d_dense(w, wd, xd, _abi.STORE_I4, 4, D.N, 8, 8, inv, shift, _abi.FN_QUANTIZED_TANH, 4, None, None)
    # the fold
    with pytest.raises(_abi.QnnError, match="dilated"):
        _abi.Fold(w, _abi.STORE_I4, 4, inv, shift, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4)
    # an in-launch projection
    pk = (D.codes(np.random.default_rng(2), (1, 1, 32, 64), -8, 7) / 8.0).astype(F32)
    wp = engine._prepack({"op": "conv", "kind": "quantized", "nb": 4, "kernel": pk, "bias": None}, _abi.STORE_I4, CUDA,
                         stride=2, same_pad=True)
    px = _abi.pack(dev(np.zeros((D.N, 16, 16, 32), F32)), 32, _abi.FN_GRID, 4, _abi.STORE_I4)
    with pytest.raises(_abi.QnnError, match="dilated"):
        _abi.conv2d(w, xd, _abi.STORE_I4, 4, D.N, 8, 8, inv, shift, _abi.FN_QUANTIZED_TANH, 4, 1, _abi.STORE_I4,
                    post_scale=0.5, proj=(wp, px, 16, 16, 4))
    assert _abi.last_kernel() == "strip_i4_c64_dil"        # nothing was launched since


# ---- layers and engines ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,kind", [("QuantizedConv2D", "i4"), ("BinaryConv2D", "bin"), ("TernaryConv2D", "t2")])
def test_keras_classes_with_dilation_rate(cls, kind):
    for padding, dil in (("same", 2), ("valid", (1, 3)), ("same", (3, 2))):
        dh, dw = (dil, dil) if isinstance(dil, int) else dil
        g = gm(3, 3, dh, dw, padding, 9, 11)
        x, k, bias = D.layer_values(kind, g, 6, 8)
        x = (D.codes(np.random.default_rng(D.seed_of(g)), x.shape, -16, 16) / 8.0).astype(F32)   # any dyadic floats
        kw = dict(kernel_size=3, padding=padding, dilation_rate=dil, H=1.0)
        if kind == "i4":
            kw["nb"] = 4
        layer = getattr(qnn_amd, cls)(8, **kw)
        layer.build((None, 9, 11, 6))
        layer.set_weights([k, bias])
        y = layer(dev(x))
        assert _abi.last_kernel() == "generic"
        want = (O.conv2d(x, D.stuff(k, dh, dw), (1, 1), padding) + bias).astype(F32)
        assert tuple(y.shape) == layer.compute_output_shape(x.shape) == want.shape
        np.testing.assert_array_equal(host(y), want)


def residual_spec(dil):
    """3 -> 16 stem, a 16 -> 16 int4 pair with the add, average pool, dense; dil = None: the zero-stuffed twin."""
    rng = np.random.default_rng(11)

    def conv(cin, cout, dst, src, dilated):
        k = (D.codes(rng, (3, 3, cin, cout), -8, 7) / 8.0).astype(F32)
        op = {"op": "conv", "kind": "quantized", "nb": 4, "kernel": k, "bias": None, "strides": (1, 1), "padding": "same",
              "src": src, "dst": dst}
        if dilated and dil is not None:
            op["dilation_rate"] = (2, 2)
        elif dilated:
            op["kernel"] = D.stuff(k, 2, 2)
        return op

    def bn(c, dst, src):
        inv, shift = bn_pow2(9 * 16, c)
        return {"op": "bn", "eps": 0.0, "gamma": np.abs(inv), "beta": shift, "mean": np.zeros(c, F32), "var": np.ones(c, F32),
                "src": src, "dst": dst}
    act = lambda dst, src: {"op": "act", "fn": "quantized_tanh", "nb": 4, "src": src, "dst": dst}      # noqa: E731
    dk = (D.codes(rng, (16, 10), -8, 7) / 8.0).astype(F32)
    return [conv(3, 16, "c0", "input", False), bn(16, "b0", "c0"), act("a0", "b0"),
            conv(16, 16, "c1", "a0", True), bn(16, "b1", "c1"), act("a1", "b1"),
            conv(16, 16, "c2", "a1", True), bn(16, "b2", "c2"),
            {"op": "add", "a": "a0", "b": "b2", "dst": "s"}, {"op": "scale", "value": 0.5, "src": "s", "dst": "h"},
            act("a2", "h"), {"op": "avgpool", "size": 8, "src": "a2", "dst": "p"}, {"op": "flatten", "src": "p", "dst": "f"},
            {"op": "dense", "kind": "quantized", "nb": 4, "kernel": dk, "bias": None, "src": "f", "dst": "d"}]


def test_engines_carry_a_dilated_residual_block():
    spec, twin = residual_spec(2), residual_spec(None)
    x = (D.codes(np.random.default_rng(4), (2, 8, 8, 3), 0, 8) / 8.0).astype(F32)
    want = O.run_spec(twin, x)
    outs = {}
    rf = engine.ResidualFusedModel(spec, first_layer="exact")
    rf.kernel_log = []
    outs["residual-fused"] = host(rf.forward(dev(x)))
    assert rf.kernel_log.count("strip_i4_c16_dil") == 2 and len(rf.kernel_log) == 3, rf.kernel_log   # one launch per conv
    outs["layers"] = host(engine.LayerModel(spec).forward(dev(x)))
    outs["graph"] = host(engine.GraphModel(spec).forward(dev(x)))
    for name, got in outs.items():
        np.testing.assert_array_equal(got, want, err_msg=name)
