"""Window, stride and padding geometry of qnn_conv2d_forward beyond 3x3 SAME, per kernel: rectangular and even windows
(SAME then pads more after than before), stride 3, strides above the window, VALID, images smaller than the window, pooling
behind odd conv maps.  The case list is tests/conv_geometry_cases.py; tests/test_conv_geometry_cpu.py proves the oracle's
convolution on it against torch in float64.

Every case runs under IMPL_AUTO and IMPL_VALU and is compared bit for bit with the oracle: all tensors are dyadic
(float32 inputs lie on the k/8 grid), so any summation order gives the same float32 and there is no tolerance in this
file.  Every case asserts _abi.last_kernel().

What the dispatch does, as the predicates say and these tests pin:
  * qnn_prepack_weights refuses a window with a side above 3 (QNN_EUNSUPPORTED), for every store.  So (4,4), (3,5), (5,5),
    (5,6), (7,7) reach no kernel at all -- neither the generic one nor, through qnn_route_gemm's `kh * kw + 3 <= 32` test,
    a tiled one -- and group 0 pins the refusal.  The window list of every other group is the part that fits.
  * The 256 x 64 / 128 / 256 tiles are therefore reached on small windows through the channel counts: Cout 128 / 256, or
    Cin 192 (three 64-channel chunks: neither the register-operand nor the weight-resident kernel takes it).
  * k_conv_ps takes k = 1 and 3 at any stride and padding where its word-count table has the layer; group 1 expects its
    name there (PS_TABLE restates the table) and `generic` everywhere else.
  * A 1x1 int4 layer with a float32 output and no activation is pw_i4_f32 before any matrix-pipe route; the groups here
    use activations, so it does not appear.
"""
import ctypes

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi, engine
from oracle import qnn_oracle as O
import conv_geometry_cases as G

pytestmark = pytest.mark.gpu
F32 = np.float32

STORE = {"f32": _abi.STORE_F32, "u8": _abi.STORE_U8, "bin": _abi.STORE_BIN, "t2": _abi.STORE_T2, "i4": _abi.STORE_I4,
         "i8": _abi.STORE_I8}
# epilogue: name -> (activation op or None, fn, act_bits, out_store)
EPI = {
    "f32": (None, _abi.FN_NONE, 0, _abi.STORE_F32),
    "q4_f32": ({"op": "act", "fn": "quantized_tanh", "nb": 4}, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_F32),
    "q4_i4": ({"op": "act", "fn": "quantized_tanh", "nb": 4}, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4),
    "q4_i8": ({"op": "act", "fn": "quantized_tanh", "nb": 4}, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I8),
    "q8_i8": ({"op": "act", "fn": "quantized_tanh", "nb": 8}, _abi.FN_QUANTIZED_TANH, 8, _abi.STORE_I8),
    "bin": ({"op": "act", "fn": "binary_tanh"}, _abi.FN_BINARY_TANH, 1, _abi.STORE_BIN),
}
# try_launch_ps's instantiations: input store -> {(words per pixel, k)}
PS_TABLE = {
    "f32": {(1, 3), (3, 3)},
    "bin": {(1, 3), (2, 3), (4, 3), (8, 3), (1, 1), (2, 1)},
    "t2": {(2, 3), (4, 3), (8, 3), (2, 1), (4, 1)},
    "i4": {(2, 3), (4, 3), (8, 3), (16, 3), (2, 1), (4, 1), (8, 1)},
    "i8": {(4, 3), (8, 3), (16, 3), (4, 1), (8, 1), (16, 1)},
}
IMPLS = (_abi.IMPL_VALU, _abi.IMPL_AUTO)          # the VALU kernels first: they are the simpler ones
SEEN = set()           # every kernel name a case of this file met (test_zz_every_family_was_reached)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def valu_name(kind, g, cin, cout, out_store):
    """The VALU route of a layer no matrix-pipe kernel is asked for: k_conv_ps where its table has it, else generic."""
    if kind == "u8":
        return "generic_u8"
    cw = cin if kind == "f32" else _abi.words(STORE[kind], cin)
    square = g["kh"] == g["kw"] and g["kh"] in (1, 3)
    if square and (cw, g["kh"]) in PS_TABLE[kind] and not (out_store == _abi.STORE_F32 and cout % 4):
        return "ps_%s_cw%d_k%d" % (kind, cw, g["kh"])
    return "generic"


def make_layer(kind, g, cin, cout, N, salt=0):
    """(x values, conv op) of one layer: dyadic values of the input store `kind` and weights of the matching width."""
    rng = np.random.default_rng(G.seed_of(g, salt) + 17 * cin + cout)
    shape_x, shape_w = (N, g["H"], g["W"], cin), (g["kh"], g["kw"], cin, cout)
    op = {"op": "conv", "strides": (g["stride"], g["stride"]), "padding": g["padding"],
          "bias": (G.codes(rng, (cout,), -8, 8) / 16.0).astype(F32)}
    if kind == "bin":
        x = (2 * G.codes(rng, shape_x, 0, 1) - 1).astype(F32)
        op.update(kind="binary", kernel=(2 * G.codes(rng, shape_w, 0, 1) - 1).astype(F32))
    elif kind == "t2":
        x = G.codes(rng, shape_x, -1, 1).astype(F32)
        op.update(kind="ternary", kernel=G.codes(rng, shape_w, -1, 1).astype(F32))
    elif kind == "i8":
        x = (G.codes(rng, shape_x, -128, 127) / 128.0).astype(F32)
        op.update(kind="quantized", nb=8, kernel=(G.codes(rng, shape_w, -128, 127) / 128.0).astype(F32))
    elif kind == "u8":
        x = G.codes(rng, shape_x, 0, 255).astype(np.uint8)
        op.update(kind="quantized", nb=4, kernel=(G.codes(rng, shape_w, -8, 7) / 8.0).astype(F32))
    else:                                                # "f32" (values on the k/8 grid) and "i4"
        x = (G.codes(rng, shape_x, -8, 7) / 8.0).astype(F32)
        op.update(kind="quantized", nb=4, kernel=(G.codes(rng, shape_w, -8, 7) / 8.0).astype(F32))
    return x, op


def bn_pow2(g, cin, cout):
    """Per-channel scale +-2^-j (odd channels negative: pooling must then take the minimum) and a dyadic shift."""
    K = g["kh"] * g["kw"] * cin
    j = max(0, int(np.ceil(np.log2(np.sqrt(K)))) - 1)
    inv = np.where(np.arange(cout) % 2 == 0, 1.0, -1.0) * 2.0 ** -j
    shift = ((np.arange(cout) % 5) - 2) / 16.0
    return inv.astype(F32), shift.astype(F32)


def run_case(kind, g, cin, cout, epis, auto, N=2, res=None, valu=None, salt=0):
    """One layer on both kernel families against the oracle.  auto / valu: the kernel name expected under IMPL_AUTO /
    IMPL_VALU (valu None: valu_name; auto None: the VALU kernel, no matrix-pipe route takes the layer).  res: None, "f32" or "packed" (int4 codes; post_scale 0.5)."""
    x, op = make_layer(kind, g, cin, cout, N, salt)
    same = g["padding"] == "same"
    use_bn = kind != "u8"                        # the byte entry has its own affine form: bias only here
    inv, shift = bn_pow2(g, cin, cout)
    if kind == "u8":
        conv = None
    else:
        conv = O.run_spec([dict(op)], x)
        assert conv.shape[1:3] == (G.out_size(g["H"], g["kh"], g["stride"], g["padding"]),
                                   G.out_size(g["W"], g["kw"], g["stride"], g["padding"]))
        conv = (conv * inv + shift).astype(F32)
    store = STORE[kind]
    wstore = _abi.STORE_F32 if kind in ("f32", "u8") else store
    abits = {"f32": 0, "u8": 0, "bin": 1, "t2": 1, "i4": 4, "i8": 8}[kind]
    xd = dev(x) if kind in ("f32", "u8") else _abi.pack(dev(x), cin, _abi.FN_GRID, abits, store)
    w = engine._prepack(op, wstore, torch.device("cuda"), stride=g["stride"], same_pad=same)
    rkw, res_val = {}, None
    if res is not None:
        assert g["pool"] == 1 and kind != "u8"
        rng = np.random.default_rng(G.seed_of(g, salt) + 5)
        res_val = (G.codes(rng, conv.shape, -8, 7) / 8.0).astype(F32)
        if res == "f32":
            rkw = dict(res=dev(res_val), res_store=_abi.STORE_F32, res_bits=0, post_scale=0.5)
        else:
            rkw = dict(res=_abi.pack(dev(res_val), cout, _abi.FN_GRID, 4, _abi.STORE_I4), res_store=_abi.STORE_I4, res_bits=4,
                       post_scale=0.5)
    Hp, Wp = G.stored_hw(g)
    try:
        for epi in epis:
            act, fn, ab, out_store = EPI[epi]
            if kind == "u8":
                want = O.u8_conv_group(x, op, None, act)
            else:
                want = conv if res_val is None else ((res_val + conv).astype(F32) * F32(0.5)).astype(F32)
                if act is not None:
                    want = O.run_spec([act], want)
            if g["pool"] == 2:
                want = O.maxpool2d(want, 2)
            assert want.shape == (N, Hp, Wp, cout)
            for impl in IMPLS:
                name = valu or valu_name(kind, g, cin, cout, out_store)
                if impl == _abi.IMPL_AUTO and auto is not None:
                    name = auto
                _abi.set_conv_impl(impl)
                y, hp, wp = _abi.conv2d(w, xd, store, abits, N, g["H"], g["W"], dev(inv) if use_bn else None,
                                        dev(shift) if use_bn else None, fn, ab, g["pool"], out_store, **rkw)
                got_name = _abi.last_kernel()
                SEEN.add((got_name, g["stride"]))
                what = "%s %s cin=%d cout=%d %s impl=%d kernel=%s" % (kind, G.geom_id(g), cin, cout, epi, impl, got_name)
                assert (hp, wp) == (Hp, Wp), what
                got = host(y) if out_store == _abi.STORE_F32 else \
                    host(_abi.unpack(y, N * hp * wp, cout, out_store, ab)).reshape(N, hp, wp, cout)
                np.testing.assert_array_equal(got, want, err_msg=what)
                assert got_name == name, what + " expected " + name
    finally:
        _abi.set_conv_impl(_abi.IMPL_AUTO)


def geoms(windows=None, **eq):
    return [g for g in G.GEOMS if G.packable(g["kh"], g["kw"]) and (windows is None or (g["kh"], g["kw"]) in windows)
            and all(g[k] == v for k, v in eq.items())]


def gm(kh, kw, stride, padding, H, W, pool=1):
    g = dict(kh=kh, kw=kw, stride=stride, padding=padding, H=H, W=W, pool=pool)
    assert G.legal(g), g
    return g


# ---- group 0: windows the library does not take ----------------------------------------------------------------------
@pytest.mark.parametrize("window", [w for w in G.WINDOWS if not G.packable(*w)], ids=lambda w: "%dx%d" % w)
def test_group0_a_window_side_above_three_is_refused_at_prepack(window):
    kh, kw = window
    for kind, cin, cout in (("f32", 3, 4), ("i4", 64, 64), ("i8", 64, 64), ("bin", 24, 10)):
        g = dict(kh=kh, kw=kw, stride=1, padding="same", H=2, W=3, pool=1)
        _, op = make_layer(kind, g, cin, cout, 1)
        with pytest.raises(_abi.QnnError, match="larger than 3x3 is not supported"):
            engine._prepack(op, _abi.STORE_F32 if kind == "f32" else STORE[kind], torch.device("cuda"))
    layer = qnn_amd.QuantizedConv2D(4, kernel_size=window, nb=4, padding="same", use_bias=False)
    with pytest.raises(_abi.QnnError, match="larger than 3x3 is not supported"):
        layer(dev(np.zeros((1, 8, 8, 3), F32)))


# ---- group 1: the generic kernel (and k_conv_ps where its table has the layer), every input store -------------------
GROUP1 = {"f32": (5, 10, ("f32", "q4_i4")), "u8": (5, 4, ("f32", "q4_i4", "bin")), "bin": (24, 10, ("f32", "bin")),
          "t2": (3, 4, ("f32", "q4_i8")), "i4": (24, 10, ("q4_f32", "q4_i4")), "i8": (5, 4, ("f32", "q8_i8"))}


@pytest.mark.parametrize("kind", sorted(GROUP1))
@pytest.mark.parametrize("window", [w for w in G.WINDOWS if G.packable(*w)], ids=lambda w: "%dx%d" % w)
def test_group1_generic_kernel_on_the_whole_list(kind, window):
    cin, cout, epis = GROUP1[kind]
    for g in geoms(windows=(window,)):
        run_case(kind, g, cin, cout, epis, auto=None)


def test_group1_binary_zero_padding_contributes_nothing():
    """BIN under SAME: a padded tap adds 0, not -1 per channel.  2x2 and 2x3 on the generic kernel (k_corr_table models
    3x3 only and is not consulted there), 3x3 on k_conv_ps with the correction table, with images smaller than the window."""
    for g in geoms(windows=((2, 2), (2, 3), (3, 3)), padding="same"):
        for cin, cout in ((3, 4), (33, 10)):
            run_case("bin", g, cin, cout, ("f32",), auto=None, salt=1)
    # all-ones input and weights: the sum is the number of in-image taps times cin, anything else is a padding error
    g = gm(2, 3, 1, "same", 2, 3)
    x = np.ones((1, 2, 3, 5), F32)
    op = {"op": "conv", "kind": "binary", "kernel": np.ones((2, 3, 5, 4), F32), "strides": (1, 1), "padding": "same"}
    w = engine._prepack(op, _abi.STORE_BIN, torch.device("cuda"), stride=1, same_pad=True)
    y, _, _ = _abi.conv2d(w, _abi.pack(dev(x), 5, _abi.FN_GRID, 1, _abi.STORE_BIN), _abi.STORE_BIN, 1, 1, 2, 3)
    taps = np.array([[4, 6, 4], [2, 3, 2]], F32)             # rows 0..1 x cols -1..1 inside a 2x3 image
    assert _abi.last_kernel() == "generic"
    np.testing.assert_array_equal(host(y), np.broadcast_to((5 * taps)[None, :, :, None], (1, 2, 3, 4)))


def test_group1_residual_merge_on_the_generic_kernel():
    for kind, cin, cout, epi in (("i4", 24, 10, "q4_i4"), ("f32", 5, 10, "q4_f32"), ("bin", 24, 10, "bin")):
        for g, res in ((gm(2, 3, 2, "same", 7, 4), "packed"), (gm(3, 1, 3, "valid", 7, 4), "f32"), (gm(2, 2, 3, "same", 6, 9), "packed")):
            run_case(kind, g, cin, cout, (epi,), auto="generic", res=res)


# ---- group 2: qnn_route_gemm, int4 and int8 ----------------------------------------------------------------------
GEMM_OUT = {"i4": ("q4_f32", "q4_i4", "q4_i8"), "i8": ("q4_f32", "q4_i4", "q8_i8")}


@pytest.mark.parametrize("kind", ("i4", "i8"))
@pytest.mark.parametrize("window", ((1, 1), (1, 3), (3, 1), (2, 2), (2, 3)), ids=lambda w: "%dx%d" % w)
def test_group2_weight_resident_kernel_on_small_windows(kind, window):
    """Cin = Cout = 64, at most 12 K-steps: mfma_*_wres256x64.  N = 3: 162 rows at 6x9, so the 256-row tile is ragged."""
    kh, kw = window
    name = "mfma_%s_wres256x64" % kind
    for g in (gm(kh, kw, 1, "same", 6, 9), gm(kh, kw, 2, "valid", 7, 9), gm(kh, kw, 3, "same", 7, 4), gm(kh, kw, 2, "same", 2, 3),
              gm(kh, kw, 1, "same", 5, 7, pool=2), gm(kh, kw, 2, "same", 8, 12, pool=2)):
        run_case(kind, g, 64, 64, GEMM_OUT[kind], auto=name, N=3)
    if window == (2, 3):                                   # two 64-channel chunks: 12 K-steps, the kernel's limit
        run_case(kind, gm(2, 3, 2, "same", 7, 9), 128, 64, GEMM_OUT[kind][1:2], auto=name, N=3)
        run_case(kind, gm(2, 3, 1, "valid", 6, 9), 128, 64, GEMM_OUT[kind][1:2], auto=name, N=3)
    if window == (2, 2):                                   # three chunks of four taps: 12 K-steps again (18 is a tile's)
        run_case(kind, gm(2, 2, 1, "same", 2, 3), 192, 64, GEMM_OUT[kind], auto=name, N=3)


@pytest.mark.parametrize("kind", ("i4", "i8"))
def test_group2_register_operand_kernel_at_stride_2_and_3_and_valid(kind):
    name = "mfma_%s_areg64x64" % kind
    for g in (gm(3, 3, 2, "same", 6, 9), gm(3, 3, 2, "same", 7, 4), gm(3, 3, 3, "same", 7, 4), gm(3, 3, 3, "same", 6, 9),
              gm(3, 3, 1, "valid", 7, 9), gm(3, 3, 2, "valid", 7, 9), gm(3, 3, 3, "valid", 6, 9), gm(3, 3, 1, "valid", 3, 3),
              gm(3, 3, 2, "same", 2, 3), gm(3, 3, 2, "same", 8, 12, pool=2), gm(3, 3, 1, "valid", 7, 9, pool=2)):
        run_case(kind, g, 64, 64, GEMM_OUT[kind], auto=name, N=3)
    for g, res in ((gm(3, 3, 2, "same", 7, 4), "packed"), (gm(3, 3, 3, "valid", 6, 9), "f32"), (gm(3, 3, 2, "valid", 7, 9), "packed")):
        run_case(kind, g, 64, 64, GEMM_OUT[kind][:2], auto=name, N=3, res=res)
    run_case(kind, gm(3, 3, 2, "valid", 7, 9), 128, 64, GEMM_OUT[kind][1:2], auto=name, N=3)          # kc = 2


@pytest.mark.parametrize("kind", ("i4", "i8"))
def test_group2_tiles_on_small_windows(kind):
    """256 x 64: Cin 192 (three chunks; 18 / 27 K-steps).  256 x 128 and 256 x 256: Cout 128 / 256 on 2x2."""
    outs = GEMM_OUT[kind]
    for g in (gm(2, 3, 2, "valid", 7, 9), gm(2, 3, 1, "same", 5, 7, pool=2), gm(3, 3, 3, "same", 7, 4), gm(2, 3, 1, "same", 2, 3)):
        run_case(kind, g, 192, 64, outs, auto="mfma_%s_256x64" % kind, N=3)
    for cout in (128, 256):
        for g in (gm(2, 2, 1, "same", 6, 9), gm(2, 2, 3, "same", 7, 4), gm(2, 2, 2, "valid", 7, 9), gm(2, 2, 1, "same", 5, 7, pool=2)):
            run_case(kind, g, 64, cout, outs + ("bin",), auto="mfma_%s_256x%d" % (kind, cout), N=3)
    run_case(kind, gm(2, 3, 2, "same", 7, 9), 128, 128, outs[1:2], auto="mfma_%s_256x128" % kind, N=3)


# ---- group 3: the stride-2 strip kernels under VALID (pt = pl = 0 and a smaller output), SAME as the control ----------
@pytest.mark.parametrize("kind", ("i4", "i8"))
@pytest.mark.parametrize("cin", (16, 32))
def test_group3_strip_stride_2_valid(kind, cin):
    epi = "q4_i4" if kind == "i4" else "q8_i8"
    for cout in (32, 64):
        for g in (gm(3, 3, 2, "valid", 7, 9), gm(3, 3, 2, "valid", 8, 8), gm(3, 3, 2, "valid", 3, 3),
                  gm(3, 3, 2, "same", 8, 8), gm(3, 3, 2, "same", 7, 9)):
            run_case(kind, g, cin, cout, (epi,), auto="strip_%s_c%d_s2" % (kind, cin), N=3)


# ---- group 4: k_conv_ps at stride 3 and VALID, channel counts that do not fill the packing word ----------------------
@pytest.mark.parametrize("kind", ("bin", "t2", "i4", "i8"))
def test_group4_pixel_stationary_kernel_at_stride_3(kind):
    cin = {"bin": 33, "t2": 33, "i4": 33, "i8": 33}[kind]       # 2 BIN words, 4 T2 words, 5 int4 words (no instance), 9 int8
    epi = {"bin": "bin", "t2": "q4_i8", "i4": "q4_i4", "i8": "q8_i8"}[kind]
    for k in (1, 3):
        for c in (cin, 80) if kind in ("bin", "t2") else (16, 30) if kind == "i4" else (14, 30):
            for g in (gm(k, k, 3, "valid", 7, 9), gm(k, k, 3, "valid", 6, 9), gm(k, k, 3, "same", 7, 4), gm(k, k, 2, "valid", 7, 9, pool=1)):
                run_case(kind, g, c, 10, ("f32", epi), auto=None, salt=2)
    assert any(n.startswith("ps_%s_" % kind) and n.endswith("_k3") and s == 3 for n, s in SEEN), sorted(SEEN)


# ---- group 5: float32 first-layer routes ------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", (1, 3))
def test_group5_float32_first_layer_off_the_lds_shape(cin):
    for cout in (64, 128):
        for g in (gm(3, 3, 2, "same", 6, 9), gm(3, 3, 2, "same", 7, 4), gm(3, 3, 3, "same", 7, 4), gm(3, 3, 1, "valid", 7, 9),
                  gm(3, 3, 2, "valid", 7, 9), gm(3, 3, 3, "valid", 6, 9), gm(3, 3, 2, "same", 8, 12, pool=2)):
            run_case("f32", g, cin, cout, ("f32", "q4_i4", "bin"), auto="mfma_f32_first_cin%d" % cin)
    # other windows on the same channels: no first-layer kernel
    for g in (gm(2, 3, 2, "same", 6, 9), gm(1, 3, 1, "valid", 7, 9)):
        run_case("f32", g, cin, 64, ("f32",), auto="generic")
    run_case("u8", gm(2, 3, 2, "same", 6, 9), 3, 64, ("f32", "q4_i4"), auto="generic_u8")
    run_case("u8", gm(3, 3, 2, "valid", 7, 9), 3, 64, ("f32", "q4_i4"), auto="generic_u8")


def test_group5_float32_activations_decline_other_windows():
    """16 float32 channels: mfma_f32_act* runs 3x3 (stride 1 / 2, SAME) and 1x1 stride 2 only."""
    for g in (gm(1, 1, 1, "same", 6, 9), gm(3, 1, 1, "same", 6, 9), gm(2, 2, 2, "same", 7, 4), gm(3, 3, 1, "valid", 7, 9)):
        run_case("f32", g, 16, 16, ("f32",), auto="generic")
    run_case("f32", gm(3, 3, 2, "same", 7, 9), 16, 16, ("f32",), auto="mfma_f32_act_c16_s2", N=3)


# ---- group 6: the Keras surface -----------------------------------------------------------------------------------
@pytest.mark.parametrize("padding", G.PADDINGS)
@pytest.mark.parametrize("stride", (2, 3))
@pytest.mark.parametrize("window", ((2, 3), (3, 2), (3, 3)), ids=lambda w: "%dx%d" % w)
def test_group6_keras_layers(window, stride, padding):
    """QuantizedConv2D and BinaryConv2D with the reference's constructor arguments, with and without input_domain (the
    conv2d_f32in path).  (5,5) is refused at prepack (group 0); (3,2) and (3,3) take its place here."""
    rng = np.random.default_rng(7 + 10 * stride + window[1])
    N, H, W, C, F = 2, 7, 9, 8, 12
    x4 = (G.codes(rng, (N, H, W, C), -8, 7) / 8.0).astype(F32)
    xb = (2 * G.codes(rng, (N, H, W, C), 0, 1) - 1).astype(F32)
    kernel = (G.codes(rng, window + (C, F), -8, 7) / 8.0).astype(F32)
    kernel_b = np.where(kernel == 0, F32(0.125), kernel)         # no weight on binarize's own tie
    bias = (G.codes(rng, (F,), -8, 8) / 16.0).astype(F32)
    for domain in (None, "in"):
        q = qnn_amd.QuantizedConv2D(F, kernel_size=window, strides=(stride, stride), padding=padding, nb=4, H=1.0,
                                    kernel_lr_multiplier=1.0, input_domain=("quantized", 4) if domain else None)
        b = qnn_amd.BinaryConv2D(F, kernel_size=window, strides=(stride, stride), padding=padding, H=1.0,
                                 kernel_lr_multiplier=1.0, input_domain="binary" if domain else None)
        g = dict(kh=window[0], kw=window[1], stride=stride, padding=padding, H=H, W=W, pool=1)
        for layer, x, kn, kind, want in (
                (q, x4, kernel, "i4" if domain else "f32",
                 O.quantized_conv2d_call(x4, kernel, bias, nb=4, strides=(stride, stride), padding=padding)),
                (b, xb, kernel_b, "bin" if domain else "f32",
                 O.binary_conv2d_call(xb, kernel_b, bias, H=1.0, strides=(stride, stride), padding=padding))):
            layer.build((None, H, W, C))
            layer.set_weights([kn, bias])
            y = host(layer(dev(x)))
            assert y.shape == layer.compute_output_shape((N, H, W, C)) == want.shape, (layer.name, domain)
            np.testing.assert_array_equal(y, want, err_msg="%s domain=%s kernel=%s" % (layer.name, domain, _abi.last_kernel()))
            assert _abi.last_kernel() == valu_name(kind, g, C, F, _abi.STORE_F32), (layer.name, domain, _abi.last_kernel())


# ---- group 7: refusals ------------------------------------------------------------------------------------------------
EMPTY = ((2, 9, 3, 3, 2), (9, 2, 3, 3, 2), (1, 9, 2, 2, 2), (9, 1, 2, 2, 2), (1, 9, 3, 3, 3), (9, 2, 3, 3, 3), (2, 2, 3, 3, 2))


@pytest.mark.parametrize("shape", EMPTY, ids=lambda s: "%dx%d_k%dx%d_s%d" % s)
def test_group7_valid_with_an_image_smaller_than_the_window_is_refused(shape):
    """0 < k - in < s: the truncating quotient said one output row.  Refused by the binding, by the layer classes and by
    the library itself (called directly with a correctly sized one-row output, so the C rule is what answers)."""
    H, W, kh, kw, s = shape
    g = dict(kh=kh, kw=kw, stride=s, padding="valid", H=H, W=W, pool=1)
    assert not G.legal(g)
    for kind, cin, cout in (("i4", 64, 64), ("f32", 3, 4)):
        x, op = make_layer(kind, g, cin, cout, 1)
        store = STORE[kind]
        w = engine._prepack(op, store, torch.device("cuda"), stride=s, same_pad=False)
        xd = dev(x) if kind == "f32" else _abi.pack(dev(x), cin, _abi.FN_GRID, 4, store)
        with pytest.raises(_abi.QnnError, match="empty output"):
            _abi.conv2d(w, xd, store, 4 if kind == "i4" else 0, 1, H, W)
        # the library: one row (or column) of output is what the old rule believed in; the buffer holds a whole one
        y = torch.zeros((1, max(1, (H - kh) // s + 1 if H >= kh else 1), max(1, (W - kw) // s + 1 if W >= kw else 1), cout),
                        dtype=torch.float32, device="cuda")
        epi = _abi.make_epilogue(None, None, _abi.FN_NONE, 0, 1, _abi.STORE_F32)
        rc = _abi.load().qnn_conv2d_forward(w.handle, _abi.ptr(xd), store, 4 if kind == "i4" else 0, 1, H, W, ctypes.byref(epi),
                                            _abi.ptr(y), _abi.stream_ptr())
        assert rc == -1 and b"empty output" in _abi.load().qnn_last_error(), (rc, _abi.load().qnn_last_error())
        assert not host(y).any()
    layer = qnn_amd.QuantizedConv2D(4, kernel_size=(kh, kw), strides=(s, s), padding="valid", nb=4)
    assert 0 in layer.compute_output_shape((1, H, W, 3))[1:3]
    with pytest.raises(_abi.QnnError, match="empty output"):
        layer(dev(np.zeros((1, H, W, 3), F32)))
    blayer = qnn_amd.BinaryConv2D(4, kernel_size=(kh, kw), strides=(s, s), padding="valid", input_domain="binary")
    with pytest.raises(_abi.QnnError, match="empty output"):
        blayer(dev(np.ones((1, H, W, 3), F32)))


# ---- the families this file must have reached (runs last: pytest keeps file order) ---------------------------------
def test_zz_every_family_was_reached():
    """Needs the groups above in the same process: run the file as a whole."""
    names = {n for n, _ in SEEN}
    for need in ("generic", "generic_u8", "mfma_i4_wres256x64", "mfma_i8_wres256x64", "mfma_i4_256x64", "mfma_i4_256x128",
                 "mfma_i4_256x256", "mfma_i8_256x64", "strip_i4_c16_s2", "strip_i8_c32_s2", "mfma_f32_first_cin3"):
        assert need in names, (need, sorted(names))
    assert ("mfma_i4_areg64x64", 2) in SEEN and ("mfma_f32_first_cin3", 2) in SEEN
    assert any(n.startswith("ps_") and n.endswith("_k3") and s == 3 for n, s in SEEN)
