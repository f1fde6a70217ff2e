"""The conv dispatch's route table (kRoutes, csrc/qnn_conv.hip): one small call per route and per boundary between two routes,
pinned by the kernel name the call reports (qnn_last_kernel).  The names are those the dispatch chose before it was
written as one ordered route list; a change of route order or of a route's eligibility shows up here first."""
import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine

pytestmark = pytest.mark.gpu
F32 = np.float32
CUDA = torch.device("cuda")
QT = _abi.FN_QUANTIZED_TANH
TRICK = _abi.faithful_trick(2.0)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _weights(rng, cin, cout, k=3, store=_abi.STORE_I4, stride=1, kind="quantized", nb=4, op="conv"):
    layer = {"op": op, "kind": kind, "nb": nb, "kernel": rng.uniform(-1, 1, (k, k, cin, cout)).astype(F32),
             "bias": (rng.standard_normal(cout) * 0.05).astype(F32)}
    return engine._prepack(layer, store, CUDA, stride=stride, same_pad=True)


def _bn(rng, cout):
    return dev((rng.uniform(0.5, 1.5, cout) / 8).astype(F32)), dev((rng.standard_normal(cout) * 0.1).astype(F32))


def _packed(rng, shape, store, bits=4):
    """Packed activations of `shape` (..., C): int4 / int8 codes of `bits`, BIN signs or T2 {-1, 0, 1}."""
    v = rng.standard_normal(shape).astype(F32)
    if store == _abi.STORE_BIN:
        return _abi.pack(dev(v), shape[-1], _abi.FN_BINARY_TANH, 1, store)
    if store == _abi.STORE_T2:
        return _abi.pack(dev(np.clip(np.round(v), -1, 1).astype(F32)), shape[-1], _abi.FN_GRID, 1, store)
    return _abi.pack(dev(v), shape[-1], QT, bits, store)


def _image(rng, shape):
    """float32 image bytes / 255: inside the domain of every restricted-domain first-layer kernel."""
    return dev((rng.integers(0, 256, shape).astype(F32) / F32(255)).astype(F32))


class epi_flags:
    """QNN_EPI_* kernel-selection flags on the calls made through _abi (None: leave them as they are)."""

    def __init__(self, flags):
        self.flags = flags

    def __enter__(self):
        self.saved = _abi._default_flags
        if self.flags is not None:
            _abi._default_flags = self.flags

    def __exit__(self, *a):
        _abi._default_flags = self.saved


class impl:
    def __init__(self, which):
        self.which = which

    def __enter__(self):
        _abi.set_conv_impl(self.which)

    def __exit__(self, *a):
        _abi.set_conv_impl(_abi.IMPL_AUTO)


def _conv_i4(cin, cout, H, W, n=2, stride=1, pool=1, out_store=_abi.STORE_I4, res=None, flags=None, fold=False,
             trick=False, k=3, x_store=_abi.STORE_I4):
    rng = np.random.default_rng(cin * 7 + cout + H + W)
    w = _weights(rng, cin, cout, k, x_store, stride)
    inv, shift = _bn(rng, cout)
    xp = _packed(rng, (n, H, W, cin), x_store)
    fn, ab = (QT, 4) if out_store != _abi.STORE_F32 else (_abi.FN_NONE, 0)
    kw = {}
    if res is not None:
        Ho, Wo = -(-H // stride), -(-W // stride)
        if res == _abi.STORE_F32:
            kw = dict(res=dev(rng.standard_normal((n, Ho, Wo, cout)).astype(F32)), res_store=_abi.STORE_F32)
        else:
            kw = dict(res=_packed(rng, (n, Ho, Wo, cout), res), res_store=res, res_bits=4)
        kw["post_scale"] = 0.5
    if fold:
        kw["fold"] = _abi.Fold.try_prepare(w, x_store, 4, inv, shift, fn, ab, out_store, **kw)
        assert kw["fold"] is not None and kw["fold"].usable
    if trick:
        kw["trick"] = TRICK
    with epi_flags(flags):
        _abi.conv2d(w, xp, x_store, 4, n, H, W, inv, shift, fn, ab, pool, out_store, **kw)
    return _abi.last_kernel()


def _conv_bin(cin, cout, H, W, pool=1, res=False, trick=False):
    rng = np.random.default_rng(cin + cout + H)
    w = _weights(rng, cin, cout, 3, _abi.STORE_BIN, kind="binary")
    xp = _packed(rng, (2, H, W, cin), _abi.STORE_BIN)
    kw = {}
    if res:
        kw = dict(res=dev(rng.standard_normal((2, H, W, cout)).astype(F32)), res_store=_abi.STORE_F32)
    if trick:
        kw["trick"] = TRICK
    _abi.conv2d(w, xp, _abi.STORE_BIN, 1, 2, H, W, None, None, _abi.FN_BINARY_TANH, 0, pool, _abi.STORE_BIN, **kw)
    return _abi.last_kernel()


def _conv_f32(cin, cout, H, W, x_store=_abi.STORE_F32, pool=1, out_store=_abi.STORE_F32, fn=_abi.FN_NONE, res=False,
              nb=4):
    rng = np.random.default_rng(cin + cout + H + W + x_store)
    w = _weights(rng, cin, cout, 3, _abi.STORE_F32, nb=nb)
    x = _image(rng, (2, H, W, cin))
    ab = 4 if fn == QT else 0
    kw = dict(res=dev(rng.standard_normal((2, H, W, cout)).astype(F32)), res_store=_abi.STORE_F32) if res else {}
    _abi.conv2d(w, x, x_store, 0, 2, H, W, None, None, fn, ab, pool, out_store, **kw)
    return _abi.last_kernel()


def _conv_u8(H, W, pool=2):
    rng = np.random.default_rng(H + W)
    w = _weights(rng, 3, 64, 3, _abi.STORE_F32)
    x = dev(rng.integers(0, 256, (2, H, W, 3)).astype(np.uint8))
    out = _abi.STORE_I4 if pool == 2 else _abi.STORE_F32
    _abi.conv2d(w, x, _abi.STORE_U8, 0, 2, H, W, None, None, QT if pool == 2 else _abi.FN_NONE, 4 if pool == 2 else 0,
                pool, out)
    return _abi.last_kernel()


def _dense(store, K, units=10, fn=_abi.FN_NONE, res=False, kind="quantized", nb=4):
    rng = np.random.default_rng(K + units + store)
    w = _weights(rng, K, units, 1, store, kind=kind, nb=nb, op="dense")
    if store == _abi.STORE_F32:
        x, bits = dev(rng.standard_normal((2, K)).astype(F32)), 0
    else:
        x, bits = _packed(rng, (2, K), store), (1 if store in (_abi.STORE_BIN, _abi.STORE_T2) else 4)
    kw = dict(res=dev(rng.standard_normal((2, units)).astype(F32)), res_store=_abi.STORE_F32) if res else {}
    epi = _abi.make_epilogue(None, None, fn, 0, 1, _abi.STORE_F32, **kw)
    y = torch.empty((2, units), dtype=torch.float32, device="cuda")
    _abi.check(_abi.load().qnn_dense_forward(w.handle, _abi.ptr(x), store, bits, 2, _abi.ctypes.byref(epi), _abi.ptr(y),
                                             _abi.stream_ptr()), "qnn_dense_forward")
    return _abi.last_kernel()


def _f32in(pref=_abi.IMPL_AUTO):
    rng = np.random.default_rng(5)
    w = _weights(rng, 64, 64, 3, _abi.STORE_BIN, kind="binary")
    x = dev(rng.standard_normal((2, 8, 8, 64)).astype(F32))
    with impl(pref):
        _abi.conv2d_f32in(w, x, _abi.FN_BINARY_TANH, 1)
    return _abi.last_kernel()


def _head(pref=_abi.IMPL_AUTO):
    rng = np.random.default_rng(6)
    wc = _weights(rng, 64, 64, 3)
    wd = _weights(rng, 1024, 10, 1, op="dense")
    inv, shift = _bn(rng, 64)
    xp = _packed(rng, (2, 8, 8, 64), _abi.STORE_I4)
    with impl(pref):
        y = _abi.conv2d_dense(wc, wd, xp, _abi.STORE_I4, 4, 2, 8, 8, inv, shift, QT, 4, None, None)
    return _abi.last_kernel() if y is not None else None


NO_STRIP, NO_STRIP64, NO_HALO, NO_LDS16 = _abi.EPI_NO_STRIP, _abi.EPI_NO_STRIP64, _abi.EPI_NO_HALO, _abi.EPI_NO_LDS16
VALU, MFMA = _abi.IMPL_VALU, _abi.IMPL_MFMA
S = _abi

# (id, implementation preference, call, kernel name)
ROUTES = [
    # 1, 2: dense layers
    ("dense_bin", 0, lambda: _dense(S.STORE_BIN, 128, kind="binary"), "dense_bin"),
    ("dense_t2", 0, lambda: _dense(S.STORE_T2, 128, kind="ternary"), "dense_t2"),
    ("dense_i4", 0, lambda: _dense(S.STORE_I4, 64), "dense_i4"),
    ("dense_i4_valu", VALU, lambda: _dense(S.STORE_I4, 64), "dense_i4"),
    ("dense_i8", 0, lambda: _dense(S.STORE_I8, 64, nb=8), "dense_i8"),
    ("dense_kwords_odd", 0, lambda: _dense(S.STORE_BIN, 32, 16, kind="binary"), "ps_bin_cw1_k1"),
    ("dense_i4_res", 0, lambda: _dense(S.STORE_I4, 64, res=True), "generic"),
    ("dense_i4_leaky", 0, lambda: _dense(S.STORE_I4, 64, fn=S.FN_LEAKY_RELU), "generic"),
    ("dense_f32", 0, lambda: _dense(S.STORE_F32, 40), "dense_f32"),
    ("dense_f32_valu", VALU, lambda: _dense(S.STORE_F32, 40), "dense_f32"),
    ("dense_f32_leaky", 0, lambda: _dense(S.STORE_F32, 40, fn=S.FN_LEAKY_RELU), "generic"),
    # 3: 1x1 strides-2 int4 -> float32 (the two-launch projection shortcut)
    ("pw", 0, lambda: _conv_i4(16, 32, 8, 8, stride=2, k=1, out_store=S.STORE_F32), "pw_i4_f32"),
    ("pw_valu", VALU, lambda: _conv_i4(16, 32, 8, 8, stride=2, k=1, out_store=S.STORE_F32), "pw_i4_f32"),
    ("pw_trick", 0, lambda: _conv_i4(16, 32, 8, 8, stride=2, k=1, out_store=S.STORE_F32, trick=True), "ps_i4_cw2_k1"),
    ("pw_res", 0, lambda: _conv_i4(16, 32, 8, 8, stride=2, k=1, out_store=S.STORE_F32, res=S.STORE_F32), "ps_i4_cw2_k1"),
    # 4: uint8 images
    ("u8", 0, lambda: _conv_u8(16, 32), "mfma_i8_first_u8"),
    ("u8_valu", VALU, lambda: _conv_u8(16, 32), "generic_u8"),
    ("u8_w_not_16", 0, lambda: _conv_u8(16, 24), "generic_u8"),
    # 5, 7: float32 first layer, first_mode 0 / 1 / 2
    ("img255", 0, lambda: _conv_f32(3, 64, 16, 32, S.STORE_F32_IMAGE, fn=QT, pool=2, out_store=S.STORE_I4),
     "mfma_i8_first_img255"),
    ("img255_valu", VALU, lambda: _conv_f32(3, 64, 16, 32, S.STORE_F32_IMAGE, fn=QT, pool=2, out_store=S.STORE_I4),
     "ps_f32_cw3_k3"),
    ("img255_w_not_16", 0, lambda: _conv_f32(3, 64, 16, 24, S.STORE_F32_IMAGE), "mfma_f32_first_cin3"),
    ("first_exact", 0, lambda: _conv_f32(3, 64, 16, 32), "mfma_f32_first_cin3"),
    ("first_exact_mfma", MFMA, lambda: _conv_f32(3, 64, 16, 32), "mfma_f32_first_cin3"),
    ("first_exact_res", 0, lambda: _conv_f32(3, 64, 16, 32, res=True), "ps_f32_cw3_k3"),
    ("first_fixed", 0, lambda: _conv_f32(3, 64, 16, 32, S.STORE_F32_UNIT, fn=QT, pool=2, out_store=S.STORE_I4),
     "mfma_i8x3_first_fixed"),
    ("first_fixed_cout128", 0, lambda: _conv_f32(3, 128, 16, 32, S.STORE_F32_UNIT), "mfma_f32_first_cin3"),
    ("first_leaky", 0, lambda: _conv_f32(3, 64, 16, 32, fn=S.FN_LEAKY_RELU), "generic"),
    # 6: the ResNet stem
    ("stem", 0, lambda: _conv_f32(3, 16, 16, 16, fn=QT, out_store=S.STORE_I4), "mfma_f32_stem_cin3"),
    ("stem_valu", VALU, lambda: _conv_f32(3, 16, 16, 16, fn=QT, out_store=S.STORE_I4), "ps_f32_cw3_k3"),
    # 8: the strip and small kernels
    ("strip16", 0, lambda: _conv_i4(16, 16, 8, 16), "strip_i4_c16"),
    ("strip16_fold", 0, lambda: _conv_i4(16, 16, 8, 16, fold=True), "strip_i4_c16_lds"),
    ("strip16_fold_no_lds16", 0, lambda: _conv_i4(16, 16, 8, 16, fold=True, flags=NO_LDS16), "strip_i4_c16"),
    ("strip16_valu", VALU, lambda: _conv_i4(16, 16, 8, 16), "ps_i4_cw2_k3"),
    ("strip16_trick", 0, lambda: _conv_i4(16, 16, 8, 16, trick=True), "ps_i4_cw2_k3"),
    ("strip16_pool2", 0, lambda: _conv_i4(16, 16, 8, 16, pool=2), "ps_i4_cw2_k3"),
    ("strip32_res_i4", 0, lambda: _conv_i4(32, 32, 8, 16, res=S.STORE_I4), "strip_i4_c32"),
    ("strip32_res_f32", 0, lambda: _conv_i4(32, 32, 8, 16, res=S.STORE_F32), "strip_i4_c32"),
    ("strip_s2", 0, lambda: _conv_i4(16, 32, 8, 16, stride=2), "strip_i4_c16_s2"),
    ("strip64", 0, lambda: _conv_i4(64, 64, 8, 16), "strip_i4_c64"),
    ("small16", 0, lambda: _conv_i4(16, 16, 8, 16, flags=NO_STRIP), "mfma_i4_small_c16"),
    ("small16_res", 0, lambda: _conv_i4(16, 16, 8, 16, flags=NO_STRIP, res=S.STORE_I4), "mfma_i4_small_c16"),
    ("small16_w_not_16", 0, lambda: _conv_i4(16, 16, 8, 24, flags=NO_STRIP), "ps_i4_cw2_k3"),
    # 9: the tiled GEMM family
    ("no_strip64_areg", 0, lambda: _conv_i4(64, 64, 8, 16, flags=NO_STRIP64), "mfma_i4_areg64x64"),
    ("no_strip64_areg_res", 0, lambda: _conv_i4(64, 64, 8, 16, flags=NO_STRIP64, res=S.STORE_I4), "mfma_i4_areg64x64"),
    ("halo", 0, lambda: _conv_i4(64, 64, 8, 16, pool=2), "mfma_i4_halo64x64"),
    ("halo_mfma", MFMA, lambda: _conv_i4(64, 64, 8, 16, pool=2), "mfma_i4_halo64x64"),
    ("halo_valu", VALU, lambda: _conv_i4(64, 64, 8, 16, pool=2), "ps_i4_cw8_k3"),
    ("no_halo", 0, lambda: _conv_i4(64, 64, 8, 16, pool=2, flags=NO_HALO), "mfma_i4_areg64x64"),
    ("areg_i8", 0, lambda: _conv_i4(64, 64, 8, 16, pool=2, x_store=S.STORE_I8), "mfma_i8_areg64x64"),
    ("wres", 0, lambda: _conv_i4(64, 64, 8, 16, k=1), "mfma_i4_wres256x64"),
    ("tile", 0, lambda: _conv_i4(128, 128, 8, 16), "mfma_i4_256x128"),
    # (Cin = 64, un-pooled, output in the input's store: the strip kernels come first; NO_STRIP64 is their per-call switch)
    ("tile_i4_256", 0, lambda: _conv_i4(64, 256, 8, 16, flags=NO_STRIP64), "mfma_i4_256x256"),
    ("tile_i8_256", 0, lambda: _conv_i4(64, 256, 8, 16, x_store=S.STORE_I8, flags=NO_STRIP64), "mfma_i8_256x256"),
    ("tile_i8_128", 0, lambda: _conv_i4(64, 128, 8, 16, x_store=S.STORE_I8, flags=NO_STRIP64), "mfma_i8_256x128"),
    ("tile_i4_192", 0, lambda: _conv_i4(64, 192, 8, 16, flags=NO_STRIP64), "mfma_i4_256x64"),
    ("tile_res", 0, lambda: _conv_i4(128, 128, 8, 16, res=S.STORE_I4), "ps_i4_cw16_k3"),
    # 10, 11: XNOR and the pixel-stationary kernels
    ("xnor_pk", 0, lambda: _conv_bin(64, 64, 8, 8), "xnor_pk_cw2"),
    ("xnor_pk_valu", VALU, lambda: _conv_bin(64, 64, 8, 8), "xnor_pk_cw2"),
    ("xnor_pk_pool2", 0, lambda: _conv_bin(64, 64, 8, 8, pool=2), "xnor_pk_cw2"),
    ("xnor_pk_trick", 0, lambda: _conv_bin(64, 64, 8, 8, trick=True), "ps_bin_cw2_k3"),
    ("xnor_pk_res", 0, lambda: _conv_bin(64, 64, 8, 8, res=True), "ps_bin_cw2_k3"),
    # 12: float32 activations on the f32 matrix pipe
    ("f32act", 0, lambda: _conv_f32(16, 16, 8, 8), "mfma_f32_act_c16"),
    ("f32act_leaky", 0, lambda: _conv_f32(16, 16, 8, 8, fn=S.FN_LEAKY_RELU), "mfma_f32_act_c16"),
    ("f32act_leaky_pool2", 0, lambda: _conv_f32(16, 16, 8, 8, fn=S.FN_LEAKY_RELU, pool=2), "mfma_f32_act_c16"),
    ("f32act_res", 0, lambda: _conv_f32(16, 16, 8, 8, res=True), "mfma_f32_act_c16"),
    ("f32act_valu", VALU, lambda: _conv_f32(16, 16, 8, 8), "generic"),
    ("f32act_image", 0, lambda: _conv_f32(16, 16, 8, 8, S.STORE_F32_IMAGE), "generic"),
    # the two entries with a route of their own
    ("f32in_xnor", 0, lambda: _f32in(), "xnor_f32_cw2"),
    ("f32in_xnor_valu", 0, lambda: _f32in(VALU), "xnor_f32_cw2"),
    ("f32in_mfma", 0, lambda: _f32in(MFMA), "ps_bin_cw2_k3"),
    ("head", 0, lambda: _head(), "mfma_i4_halo64x64+dense"),
    ("head_valu", 0, lambda: _head(VALU), None),
]


@pytest.mark.parametrize("case", ROUTES, ids=[r[0] for r in ROUTES])
def test_route_table(case):
    _, pref, call, want = case
    with impl(pref):
        got = call()
    assert got == want, (got, want)


# Every kernel the tiled GEMM translation unit (csrc/qnn_mfma.hip) emits: 32x32x32 on the 256 x 64 tile (Cout = 192) and for
# 1-bit outputs, 16x16x64 on 256 x 128 / 256 x 256 (Cout = 128 / 256) for int4 inputs, its LDS-DMA form for int8 inputs.
# No combination is skipped: each output store is called with an activation check_epilogue accepts for it (BIN needs
# binary_tanh).
GEMM_OUT = {S.STORE_F32: (S.FN_NONE, 0), S.STORE_BIN: (S.FN_BINARY_TANH, 0), S.STORE_I4: (QT, 4), S.STORE_I8: (QT, 8)}
GEMM_TILE = {192: 64, 128: 128, 256: 256}
GEMM_CASES = [(xs, cout, out, pool) for xs in (S.STORE_I4, S.STORE_I8) for cout in (192, 128, 256)
              for out in (S.STORE_F32, S.STORE_BIN, S.STORE_I4, S.STORE_I8) for pool in (1, 2)]
_gemm_layers = {}


def _gemm_layer(xs, cout):
    """Weights, BN vectors and the packed inputs (N = 2 and N = 3) of one (input store, Cout): built once."""
    if (xs, cout) not in _gemm_layers:
        rng = np.random.default_rng(1000 * xs + cout)
        bits = 4 if xs == S.STORE_I4 else 8
        w = _weights(rng, 64, cout, 3, xs, nb=bits)
        _gemm_layers[xs, cout] = (w, _bn(rng, cout), bits,
                                  {n: _abi.pack(dev(rng.standard_normal((n, 8, 16, 64)).astype(F32)), 64, QT, bits, xs)
                                   for n in (2, 3)})
    return _gemm_layers[xs, cout]


@pytest.mark.parametrize("xs,cout,out,pool", GEMM_CASES,
                         ids=["i%d_c%d_out%d_pool%d" % c for c in GEMM_CASES])
def test_gemm_tiles_match_valu(xs, cout, out, pool):
    """8 x 16 pixels, 3x3, Cin = 64.  N = 2 fills the 256-row tile exactly (256 conv rows; pooled: 64 windows = 256 rows),
    N = 3 leaves a ragged second tile (384 rows).  Bit for bit against k_conv_ps (IMPL_VALU), an independent kernel.
    QNN_EPI_NO_STRIP64 keeps the un-pooled int4 -> int4 and int8 -> int8 calls off the Cin = 64 strip kernels, which come
    first in the route list; it changes nothing for the other calls."""
    w, (inv, shift), bits, xp = _gemm_layer(xs, cout)
    fn, ab = GEMM_OUT[out]
    for n in (2, 3):
        got = {}
        for pref in (_abi.IMPL_AUTO, VALU):
            with impl(pref), epi_flags(NO_STRIP64):
                y = _abi.conv2d(w, xp[n], xs, bits, n, 8, 16, inv, shift, fn, ab, pool, out)[0]
            got[pref] = (_abi.last_kernel(), y.cpu().numpy())
        assert got[_abi.IMPL_AUTO][0] == "mfma_i%d_256x%d" % (bits, GEMM_TILE[cout]), got[_abi.IMPL_AUTO][0]
        assert got[VALU][0] == "ps_i%d_cw%d_k3" % (bits, 64 * bits // 32), got[VALU][0]
        assert got[_abi.IMPL_AUTO][1].shape == got[VALU][1].shape
        assert np.array_equal(got[_abi.IMPL_AUTO][1], got[VALU][1]), (n, np.count_nonzero(got[_abi.IMPL_AUTO][1] != got[VALU][1]))
