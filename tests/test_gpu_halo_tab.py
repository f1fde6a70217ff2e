"""k_conv_mfma_halo (csrc/qnn_mfma_areg.hip) fed from the handles: the FP6 filter image in LDS order (k_fp6_weights), the
per-lane epilogue table of a mode-2 fold (qnn_fold.h, qnn_halo_epi_entry; QNN_EPI_NO_HALO_TAB = set_option("halo_tab", 0)
keeps the in-kernel preamble), the classifier table copied in 16-byte pieces, and the conv + classifier form on the FP6
matrix pipe.

Every launch runs under the four combinations of halo_tab and fp6 and is compared, with no tolerance, with the default
launch and with the oracle; the kernel tag is asserted.  BN scales are mixed, all positive and all negative.
The dispatch gives the halo kernel the layers with ONE 64-filter slice (tests/test_gpu_halo.py, test_gpu_halo_pool.py
record mfma_i4_256x128 for 128 filters), so the two-slice case checks that its handle -- which does carry a two-slice
table and image -- runs on that kernel with the same codes.
A batch larger than DISTINCT repeats DISTINCT images cyclically: the oracle evaluates DISTINCT images whatever N is.
"""
import itertools
import zlib

import numpy as np
import pytest
import torch

import qnn_amd  # noqa: F401
from qnn_amd import _abi, engine, nets
from oracle import qnn_oracle as O
from test_gpu_halo import CASES
from test_gpu_halo_fp6 import TILED, _want
from test_gpu_parity import Q, dev, host

pytestmark = pytest.mark.gpu
F32 = np.float32
DISTINCT = 13
COMBOS = list(itertools.product((1, 0), (1, 0)))            # (halo_tab, fp6); the first is the default
SIGNS = [None, 1.0, -1.0]
HALO, HEAD = "mfma_i4_halo64x64", "mfma_i4_halo64x64+dense"


class _Flags:
    def __init__(self, tab, fp6):
        self.v = (tab, fp6)

    def __enter__(self):
        _abi.set_option("halo_tab", self.v[0])
        _abi.set_option("fp6", self.v[1])

    def __exit__(self, *a):
        _abi.set_option("halo_tab", 1)
        _abi.set_option("fp6", 1)


def _layer(rng, cin=64, cout=64, gamma_sign=None, codes_w=None):
    k = rng.uniform(-1, 1, (3, 3, cin, cout)).astype(F32) if codes_w is None else (codes_w / F32(8)).astype(F32)
    op = {"op": "conv", "kind": "quantized", "nb": 4, "kernel": k, "strides": (1, 1), "padding": "same",
          "bias": (rng.standard_normal(cout) * 0.5).astype(F32)}
    g = rng.uniform(0.5, 1.5, cout).astype(F32) * (rng.choice([-1.0, 1.0], cout) if gamma_sign is None else F32(gamma_sign))
    bn = {"gamma": g.astype(F32), "beta": (rng.standard_normal(cout) * 4).astype(F32),
          "mean": (rng.standard_normal(cout) * 4).astype(F32), "var": rng.uniform(20 * cin / 64, 60 * cin / 64, cout).astype(F32),
          "eps": 1e-3}
    return op, bn


def _head(rng, units=10):
    dop = {"op": "dense", "kind": "quantized", "nb": 4, "kernel": rng.uniform(-1, 1, (1024, units)).astype(F32),
           "bias": (rng.standard_normal(units) * 0.1).astype(F32)}
    dbn = {"gamma": rng.uniform(0.5, 1.5, units).astype(F32), "beta": rng.standard_normal(units).astype(F32),
           "mean": rng.standard_normal(units).astype(F32), "var": rng.uniform(50, 150, units).astype(F32), "eps": 1e-3}
    return dop, dbn


class _Prepared:
    """weights, BN constants and ONE fold handle of a layer"""

    def __init__(self, op, bn, mode=2):
        self.cout = op["kernel"].shape[3]
        self.cin = op["kernel"].shape[2]
        self.w = engine._prepack(op, _abi.STORE_I4, torch.device("cuda"), stride=1, same_pad=True)
        i, s = engine.bn_constants(bn)
        self.inv, self.shift = dev(i), dev(s)
        self.f = _abi.Fold.try_prepare(self.w, _abi.STORE_I4, 4, self.inv, self.shift, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4)
        assert self.f is not None and self.f.usable and mode in (None, self.f.mode), self.f

    def conv(self, x, pool=2):
        """the folded layer under every flag combination: [(codes, tag)]"""
        N, H, W, _ = x.shape
        xp = _abi.pack(dev(x), self.cin, _abi.FN_GRID, 4, _abi.STORE_I4)
        outs = []
        for tab, fp6 in COMBOS:
            with _Flags(tab, fp6):
                y, hp, wp = _abi.conv2d(self.w, xp, _abi.STORE_I4, 4, N, H, W, self.inv, self.shift, _abi.FN_QUANTIZED_TANH,
                                        4, pool, _abi.STORE_I4, fold=self.f)
                outs.append((host(_abi.unpack(y, N * hp * wp, self.cout, _abi.STORE_I4, 4)).reshape(N, hp, wp, self.cout),
                             _abi.last_kernel()))
        return outs

    def conv_dense(self, x, dop, dbn):
        """conv + classifier in one launch under every flag combination: [(logits, tag)]"""
        N, H, W, _ = x.shape
        wd = engine._prepack(dop, _abi.STORE_I4, torch.device("cuda"))
        dinv, dshift = (dev(a) for a in engine.bn_constants(dbn))
        xp = _abi.pack(dev(x), 64, _abi.FN_GRID, 4, _abi.STORE_I4)
        outs = []
        for tab, fp6 in COMBOS:
            with _Flags(tab, fp6):
                y = _abi.conv2d_dense(self.w, wd, xp, _abi.STORE_I4, 4, N, H, W, self.inv, self.shift,
                                      _abi.FN_QUANTIZED_TANH, 4, dinv, dshift, fold=self.f)
                outs.append((host(y), _abi.last_kernel()))
        return outs


def _check(outs, want, tag):
    assert [k for _, k in outs] == [tag] * len(outs), [k for _, k in outs]
    for (got, _), combo in zip(outs, COMBOS):
        np.testing.assert_array_equal(got, outs[0][0], err_msg="(halo_tab, fp6) = %r against the default" % (combo,))
        np.testing.assert_array_equal(got, want, err_msg="(halo_tab, fp6) = %r against the oracle" % (combo,))


def _want_head(x, op, bn, dop, dbn):
    return O.run_spec([dict(op), dict(bn, op="bn"), Q(4), {"op": "maxpool", "size": 2}, {"op": "flatten"}, dict(dop),
                       dict(dbn, op="bn")], x)


def _codes(rng, shape):
    return (rng.integers(-8, 8, shape) / 8).astype(F32)


@pytest.mark.parametrize("gamma_sign", SIGNS)
@pytest.mark.parametrize("case", TILED, ids=[c[0] for c in TILED])
def test_tiled_cases(case, gamma_sign):
    name, shape, _, tag = case
    rng = np.random.default_rng(zlib.crc32(("tab" + name).encode()))
    x = _codes(rng, shape)
    op, bn = _layer(rng, gamma_sign=gamma_sign)
    _check(_Prepared(op, bn).conv(x), _want(x, op, bn), tag)


@pytest.mark.parametrize("gamma_sign", SIGNS)
def test_two_filter_slices(gamma_sign):
    """2 x 16^2 x 64 -> 128: the handle's table and image have two slices; the dispatch keeps 128 filters on the tile kernel"""
    tag = dict((c[0], c[3]) for c in CASES)["cout128"]
    rng = np.random.default_rng(11)
    x = _codes(rng, (2, 16, 16, 64))
    op, bn = _layer(rng, cout=128, gamma_sign=gamma_sign)
    _check(_Prepared(op, bn).conv(x), _want(x, op, bn), tag)


@pytest.mark.parametrize("gamma_sign", SIGNS)
def test_eight_wave_workgroups_conv(gamma_sign):
    """512 x 16^2 x 64 -> 64: 2048 tiles, eight waves per workgroup"""
    rng = np.random.default_rng(12)
    xd = _codes(rng, (DISTINCT, 16, 16, 64))
    idx = np.arange(512) % DISTINCT
    op, bn = _layer(rng, gamma_sign=gamma_sign)
    _check(_Prepared(op, bn).conv(xd[idx]), _want(xd, op, bn)[idx], HALO)


@pytest.mark.parametrize("gamma_sign", SIGNS)
@pytest.mark.parametrize("N", [2048, 3], ids=["eight_waves", "four_waves"])
def test_conv_classifier(N, gamma_sign):
    """N x 8^2 x 64 -> 64 + dense 1024 -> 10: 2048 images are the eight-wave workgroups, 3 the four-wave one"""
    rng = np.random.default_rng(13 + N)
    xd = _codes(rng, (min(N, DISTINCT), 8, 8, 64))
    idx = np.arange(N) % len(xd)
    op, bn = _layer(rng, gamma_sign=gamma_sign)
    dop, dbn = _head(rng)
    _check(_Prepared(op, bn).conv_dense(xd[idx], dop, dbn), _want_head(xd, op, bn, dop, dbn)[idx], HEAD)


@pytest.mark.parametrize("xc", [-8, 7])
@pytest.mark.parametrize("wc", [-8, 7])
def test_extreme_codes_through_the_classifier_form(xc, wc):
    """tests/test_gpu_halo_fp6.py::test_fp6_halo_extreme_codes on 8 x 8 images behind the classifier: the largest |sum|"""
    rng = np.random.default_rng(200 + 16 * xc + wc)
    x = np.full((3, 8, 8, 64), xc / 8, F32)
    x[1, :, ::3] = (-8 if xc == 7 else 7) / 8
    cw = np.full((3, 3, 64, 64), wc, F32)
    cw[..., 32:] = rng.choice([-8.0, 7.0], cw[..., 32:].shape)
    op, bn = _layer(rng, codes_w=cw)
    dop, dbn = _head(rng)
    _check(_Prepared(op, bn).conv_dense(x, dop, dbn), _want_head(x, op, bn, dop, dbn), HEAD)


@pytest.mark.parametrize("gamma_sign", SIGNS)
def test_one_handle_two_geometries(gamma_sign):
    """the table holds nothing of the geometry: one handle, 16 x 16 images (8 x 2 tiles), then 8 x 8 (4 x 4), then the head"""
    rng = np.random.default_rng(14)
    op, bn = _layer(rng, gamma_sign=gamma_sign)
    dop, dbn = _head(rng)
    p = _Prepared(op, bn)
    xa, xb = _codes(rng, (5, 16, 16, 64)), _codes(rng, (7, 8, 8, 64))
    _check(p.conv(xa), _want(xa, op, bn), HALO)
    _check(p.conv(xb), _want(xb, op, bn), HALO)
    _check(p.conv_dense(xb, dop, dbn), _want_head(xb, op, bn, dop, dbn), HEAD)


def test_handle_without_a_table_still_runs():
    """32 input channels (an un-pooled layer of the row-walking kernels): no halo table in the handle and no FP6 image;
    the flags change nothing"""
    rng = np.random.default_rng(15)
    x = _codes(rng, (3, 16, 16, 32))
    op, bn = _layer(rng, cin=32, cout=32)
    outs = _Prepared(op, bn, mode=None).conv(x, pool=1)
    assert "halo" not in outs[0][1]
    v = O.quantized_conv2d_call(x, op["kernel"], op["bias"], nb=4)
    v = O.batchnorm_inference(v, bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"])
    _check(outs, O.quantized_tanh(v, 4), outs[0][1])


def test_headline_network_same_logits_under_all_flags():
    cf = nets.baseline_config(2)
    spec = nets.build_spec(cf, nets.SEED_BASE + 2)
    x = nets.synthetic_images(cf, 96, 5)
    want = O.run_spec(spec, x, float_conv="device")
    for tab, fp6 in COMBOS:
        with _Flags(tab, fp6):
            m = engine.FusedModel(spec, first_layer="exact")
            m.kernel_log = []
            got = host(m(dev(x)))
            assert HALO in m.kernel_log and HEAD in m.kernel_log, m.kernel_log
        np.testing.assert_array_equal(got, want, err_msg="(halo_tab, fp6) = %r" % ((tab, fp6),))
