"""The FP6 (e2m3) form of k_conv_mfma_halo (csrc/qnn_mfma_areg.hip): the folded pooled int4 64-channel layers on
v_mfma_scale_f32_32x32x64_f8f6f4.  Its codes are bit-identical to the int8 form (QNN_EPI_NO_FP6, set_option("fp6", 0))
and to the oracle over the halo kernel's tilings, the extreme codes (largest |sum|), min- and max-pooled channels and the
zero padding; the kernel tag is the same for both forms.  The headline network gives the same logits either way.
"""
import zlib

import numpy as np
import pytest
import torch

import qnn_amd  # noqa: F401
from qnn_amd import _abi, engine, nets
from oracle import qnn_oracle as O
from test_gpu_halo import CASES
from test_gpu_parity import dev, host

pytestmark = pytest.mark.gpu
F32 = np.float32
TILED = [c for c in CASES if c[3] == "mfma_i4_halo64x64"]


def _layer(rng, codes_w=None, gamma_sign=None):
    k = rng.uniform(-1, 1, (3, 3, 64, 64)).astype(F32) if codes_w is None else (codes_w / F32(8)).astype(F32)
    op = {"op": "conv", "kind": "quantized", "nb": 4, "kernel": k, "strides": (1, 1), "padding": "same",
          "bias": (rng.standard_normal(64) * 0.5).astype(F32)}
    g = rng.uniform(0.5, 1.5, 64).astype(F32) * (rng.choice([-1.0, 1.0], 64) if gamma_sign is None else F32(gamma_sign))
    bn = {"gamma": g.astype(F32), "beta": (rng.standard_normal(64) * 4).astype(F32),
          "mean": (rng.standard_normal(64) * 4).astype(F32), "var": rng.uniform(20, 60, 64).astype(F32), "eps": 1e-3}
    return op, bn


def _run(x, op, bn):
    """folded launch with the FP6 form, then with the int8 form: (codes, tag) twice"""
    N, H, W, _ = x.shape
    w = engine._prepack(op, _abi.STORE_I4, torch.device("cuda"), stride=1, same_pad=True)
    i, s = engine.bn_constants(bn)
    inv, shift = dev(i), dev(s)
    f = _abi.Fold.try_prepare(w, _abi.STORE_I4, 4, inv, shift, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4)
    assert f is not None and f.usable and f.mode == 2, f
    xp = _abi.pack(dev(x), 64, _abi.FN_GRID, 4, _abi.STORE_I4)
    outs = []
    for fp6 in (1, 0):
        _abi.set_option("fp6", fp6)
        try:
            y, hp, wp = _abi.conv2d(w, xp, _abi.STORE_I4, 4, N, H, W, inv, shift, _abi.FN_QUANTIZED_TANH, 4, 2,
                                    _abi.STORE_I4, fold=f)
            outs.append((host(_abi.unpack(y, N * hp * wp, 64, _abi.STORE_I4, 4)).reshape(N, hp, wp, 64), _abi.last_kernel()))
        finally:
            _abi.set_option("fp6", 1)
    return outs


def _want(x, op, bn):
    v = O.quantized_conv2d_call(x, op["kernel"], op["bias"], nb=4)
    v = O.batchnorm_inference(v, bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"])
    return O.maxpool2d(O.quantized_tanh(v, 4))


@pytest.mark.parametrize("gamma_sign", [None, 1.0, -1.0])
@pytest.mark.parametrize("case", TILED, ids=[c[0] for c in TILED])
def test_fp6_halo_bit_exact_vs_int8_halo_and_oracle(case, gamma_sign):
    name, shape, _, kern_want = case
    rng = np.random.default_rng(zlib.crc32(("fp6" + name).encode()))
    x = (rng.integers(-8, 8, shape) / 8).astype(F32)
    op, bn = _layer(rng, gamma_sign=gamma_sign)
    (got, kern), (ref, kern_ref) = _run(x, op, bn)
    assert kern == kern_want and kern_ref == kern_want, (kern, kern_ref)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(got, _want(x, op, bn))


@pytest.mark.parametrize("xc", [-8, 7])
@pytest.mark.parametrize("wc", [-8, 7])
def test_fp6_halo_extreme_codes(xc, wc):
    """Every input code -8 or 7 against every weight code -8 or 7 (the largest |sum|, 9 * 64 * 64), an image with the
    other extreme on every third column, the zero padding on the border taps, min- and max-pooled channels."""
    rng = np.random.default_rng(200 + 16 * xc + wc)
    x = np.full((3, 16, 16, 64), xc / 8, F32)
    x[1, :, ::3] = (-8 if xc == 7 else 7) / 8
    cw = np.full((3, 3, 64, 64), wc, F32)
    cw[..., 32:] = rng.choice([-8.0, 7.0], cw[..., 32:].shape)
    op, bn = _layer(rng, codes_w=cw)
    (got, kern), (ref, _) = _run(x, op, bn)
    assert kern == "mfma_i4_halo64x64"
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(got, _want(x, op, bn))


def test_fp6_headline_network_same_logits():
    """The headline VGG (its B0 layer runs on the FP6 form) with and without it."""
    cf = nets.baseline_config(2)
    spec = nets.build_spec(cf, nets.SEED_BASE + 2)
    x = nets.synthetic_images(cf, 96, 5)
    outs = {}
    for fp6 in (1, 0):
        _abi.set_option("fp6", fp6)
        try:
            m = engine.FusedModel(spec, first_layer="exact")
            m.kernel_log = []
            outs[fp6] = host(m(dev(x)))
            assert any("halo" in k for k in m.kernel_log), m.kernel_log
        finally:
            _abi.set_option("fp6", 1)
    np.testing.assert_array_equal(outs[1], outs[0])
    np.testing.assert_array_equal(outs[1], O.run_spec(spec, x, float_conv="device"))
