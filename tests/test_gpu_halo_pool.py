"""The 2x2 pooling of k_conv_mfma_halo (csrc/qnn_mfma_areg.hip) by the sign of the BN scales, and the seeded accumulators
of its FP6 form.

A wave pools its 64-filter slice by the maximum alone when every BN scale of the slice is >= 0 and by maximum / minimum /
select otherwise: a wave-uniform branch around the epilogue.  The FP6 form starts its float32 accumulators from 1.5 * 2^23
and pools their bit patterns as integers, which is exact as long as every partial sum S + 8 sum(w) stays below 2^22 in
magnitude (the largest is 576 * 15 * 8 = 69 120).

Every case runs the folded layer three times -- the default dispatch (the FP6 form where the layer has an FP6 filter image),
QNN_EPI_NO_FP6 (the int8 form) and QNN_EPI_NO_HALO (k_conv_mfma_areg) -- asserts the kernel tag of each and compares all
three, bit for bit, with each other and with the oracle:
  * B0 and C0 geometry (16 x 16 and 8 x 8 pixels of 64 channels), 64 and 128 filters;
  * BN scales all positive, all negative, mixed inside every 64-filter slice, negative in one slice only;
  * N in {1, 3, 260, 4096}: one tile or a few, a ragged last pass of the persistent tile loop, more tiles than waves;
  * input / weight codes pinned at -8 / 7 in all four pairings (|S| up to 576 * 8 * 8, the largest |S + 8 sum(w)|).
The dispatch gives the halo kernel the layers with ONE 64-filter slice; 128 filters stay on the tile kernel
(mfma_i4_256x128, as tests/test_gpu_halo.py records), so those cases check that kernel against the same references and a
launch of the halo kernel never holds both branches: "negative in one slice only" is then, for 64 filters, the upper 32
filters of the slice (one wave's two MFMA column blocks with different signs).
A batch of N images repeats DISTINCT different ones cyclically, so the oracle evaluates DISTINCT images whatever N is.
"""
import zlib

import numpy as np
import pytest
import torch

import qnn_amd  # noqa: F401
from qnn_amd import _abi, engine
from oracle import qnn_oracle as O
from test_gpu_parity import dev, host

pytestmark = pytest.mark.gpu
F32 = np.float32
DISTINCT = 13
GEOMETRY = {"b0": (16, 16), "c0": (8, 8)}
# filters -> kernel tags of (default, QNN_EPI_NO_FP6, QNN_EPI_NO_HALO)
TAGS = {64: ("mfma_i4_halo64x64", "mfma_i4_halo64x64", "mfma_i4_areg64x64"),
        128: ("mfma_i4_256x128", "mfma_i4_256x128", "mfma_i4_256x128")}


def _signs(mode, cout):
    s = np.ones(cout, F32)
    if mode == "neg":
        s[:] = -1
    elif mode == "mixed":                                 # both signs inside every 32-filter column block
        s[np.arange(cout) % 3 == 1] = -1
    elif mode == "slice":                                 # the last 64-filter slice (64 filters: its upper half)
        s[cout - (64 if cout > 64 else 32):] = -1
    else:
        assert mode == "pos"
    return s


def _layer(rng, cout, mode, codes_w=None):
    k = rng.uniform(-1, 1, (3, 3, 64, cout)).astype(F32) if codes_w is None else (codes_w / F32(8)).astype(F32)
    op = {"op": "conv", "kind": "quantized", "nb": 4, "kernel": k, "strides": (1, 1), "padding": "same",
          "bias": (rng.standard_normal(cout) * 0.5).astype(F32)}
    bn = {"gamma": (rng.uniform(0.5, 1.5, cout).astype(F32) * _signs(mode, cout)).astype(F32),
          "beta": (rng.standard_normal(cout) * 4).astype(F32), "mean": (rng.standard_normal(cout) * 4).astype(F32),
          "var": rng.uniform(20, 60, cout).astype(F32), "eps": 1e-3}
    return op, bn


def _want(xd, op, bn, N):
    v = O.quantized_conv2d_call(xd, op["kernel"], op["bias"], nb=4)
    v = O.batchnorm_inference(v, bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"])
    return O.maxpool2d(O.quantized_tanh(v, 4))[np.arange(N) % len(xd)]


def _run(xd, op, bn, N):
    """the folded layer under the default dispatch, QNN_EPI_NO_FP6 and QNN_EPI_NO_HALO: [(codes, kernel tag)] * 3"""
    cout = op["kernel"].shape[3]
    x = xd[np.arange(N) % len(xd)]
    _, H, W, _ = x.shape
    w = engine._prepack(op, _abi.STORE_I4, torch.device("cuda"), stride=1, same_pad=True)
    i, s = engine.bn_constants(bn)
    inv, shift = dev(i), dev(s)
    f = _abi.Fold.try_prepare(w, _abi.STORE_I4, 4, inv, shift, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4)
    assert f is not None and f.usable and f.mode == 2, f
    xp = _abi.pack(dev(x), 64, _abi.FN_GRID, 4, _abi.STORE_I4)
    outs = []
    for key in (None, "fp6", "halo"):
        if key:
            _abi.set_option(key, 0)
        try:
            y, hp, wp = _abi.conv2d(w, xp, _abi.STORE_I4, 4, N, H, W, inv, shift, _abi.FN_QUANTIZED_TANH, 4, 2,
                                    _abi.STORE_I4, fold=f)
            kern = _abi.last_kernel()
            outs.append((host(_abi.unpack(y, N * hp * wp, cout, _abi.STORE_I4, 4)).reshape(N, hp, wp, cout), kern))
        finally:
            if key:
                _abi.set_option(key, 1)
    return outs


def _check(xd, op, bn, N):
    cout = op["kernel"].shape[3]
    outs = _run(xd, op, bn, N)
    assert tuple(k for _, k in outs) == TAGS[cout], [k for _, k in outs]
    want = _want(xd, op, bn, N)
    for got, kern in outs:
        np.testing.assert_array_equal(got, want, err_msg=kern)


@pytest.mark.parametrize("N", [1, 3, 260, 4096])
@pytest.mark.parametrize("mode", ["pos", "neg", "mixed", "slice"])
@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("geo", sorted(GEOMETRY))
def test_halo_pooling_by_bn_sign(geo, cout, mode, N):
    H, W = GEOMETRY[geo]
    rng = np.random.default_rng(zlib.crc32(("pool %s %d %s" % (geo, cout, mode)).encode()))
    xd = (rng.integers(-8, 8, (min(N, DISTINCT), H, W, 64)) / 8).astype(F32)
    op, bn = _layer(rng, cout, mode)
    _check(xd, op, bn, N)


@pytest.mark.parametrize("mode", ["pos", "mixed"])
@pytest.mark.parametrize("wc", [-8, 7])
@pytest.mark.parametrize("xc", [-8, 7])
@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("geo", sorted(GEOMETRY))
def test_halo_seeded_accumulators_at_the_extreme_codes(geo, cout, xc, wc, mode):
    """Every input code xc against every weight code wc: S = 576 xc wc in the interior (|S| = 576 * 8 * 8 for -8, -8) and
    S + 8 sum(w) = 576 wc (xc + 8), the seeded accumulator's largest excursions (-69 120 for xc = 7, wc = -8; 60 480 for
    7, 7).  The second image carries the other extreme on every third column, the third random codes; the upper half of
    the filters mixes the two weight extremes."""
    H, W = GEOMETRY[geo]
    rng = np.random.default_rng(zlib.crc32(("ext %s %d %d %d %s" % (geo, cout, xc, wc, mode)).encode()))
    xd = np.full((3, H, W, 64), xc / 8, F32)
    xd[1, :, ::3] = (-8 if xc == 7 else 7) / 8
    xd[2] = rng.integers(-8, 8, xd[2].shape) / 8
    cw = np.full((3, 3, 64, cout), wc, F32)
    cw[..., cout // 2:] = rng.choice([-8.0, 7.0], cw[..., cout // 2:].shape)
    op, bn = _layer(rng, cout, mode, codes_w=cw)
    _check(xd, op, bn, 3)
