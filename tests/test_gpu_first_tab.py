"""The byte first layer's folded form with its operands taken from the fold handle (csrc/qnn_first_u8.hip, qnn_fold.h).

qnn_fold_prepare builds, for a mode-3 handle, the table a launch used to derive in every wave's preamble (dealt B operands,
negated filters for negative BN scales, the two constants per channel), with the one device function the preamble itself
calls, and searches the "bits" form of the fold: accumulator seeded with 0x4B400000, an integer beta per channel in the
MFMA's offset block, one FMA per value and no conversion.  Nothing of that may move a bit.  Every launch here is compared,
on the unpacked codes with no tolerance, with

  * the same launch under QNN_EPI_NO_FIRST_TAB (set_option("first_tab", 0)): in-kernel preamble, mode-3 epilogue,
  * the un-folded kernel (fold = None),
  * and, for the small batches, the oracle's restatement of the typed entry (oracle/qnn_oracle.py, u8_conv_group),

through both entries (uint8 bytes and float32 bytes / 255).  Shapes are the smallest that reach each path of the walk.
"""
import zlib

import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine
from oracle import qnn_oracle as O
from test_gpu_parity import Q, _rand_bn, dev, host

pytestmark = pytest.mark.gpu
F32 = np.float32
MAGIC = 0x4B400000

# (N, H, W): two strips per row and more than one task per wave of a small grid; one strip with both edge columns;
# one step; an odd number of steps (the rp < rp1 tail); more tasks than one workgroup has waves
SHAPES = [(3, 32, 32), (5, 16, 16), (2, 4, 16), (2, 6, 16), (70, 32, 32)]


def _bn(rng, signs, scale=27 * 0.3):
    bn = _rand_bn(rng, 64, scale)
    g = np.abs(bn["gamma"])
    if signs == "neg":
        g = -g
    elif signs == "mixed":
        g = g * np.where((np.arange(64) * 7) % 5 < 2, -1.0, 1.0)         # differs inside every group of four channels
    bn["gamma"] = g.astype(F32)
    return bn


def _prepare(w, inv, shift, bits=True):
    _abi.set_option("first_bits", 1 if bits else 0)
    try:
        f = _abi.Fold.try_prepare(w, _abi.STORE_U8, 0, inv, shift, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4)
    finally:
        _abi.set_option("first_bits", 1)
    assert f is not None and f.mode == 3 and f.usable, (f and (f.mode, f.folded))
    return f


def _layer(rng, kernel, signs, bias, bits=True):
    """(op, bn, weights, inv, shift, handle); bits = False: prepared under QNN_EPI_NO_FIRST_BITS.
    The bits search finds nothing on about one channel in a thousand (its candidates bunch where one ulp of C' is close to
    a simple fraction of a step of S), and one such channel keeps the whole table on mode 3: the BN statistics are drawn
    again, at most three times, until the handle has the form these tests are about.  The fallback has its own test."""
    op = {"op": "conv", "kind": "quantized", "nb": 4, "kernel": kernel.astype(F32), "strides": (1, 1), "padding": "same"}
    if bias:
        op["bias"] = (rng.standard_normal(64) * 0.05).astype(F32)
    w = engine._prepack(op, _abi.STORE_F32, torch.device("cuda"), stride=1, same_pad=True)
    for _ in range(4):
        bn = _bn(rng, signs)
        inv, shift = (dev(a) for a in engine.bn_constants(bn))
        f = _prepare(w, inv, shift, bits)
        if not bits or _table_has_bits(f):
            break
    return op, bn, w, inv, shift, f


def _table_has_bits(f):
    """qnn_fold_constants: beta of a mode-3 handle is the bits form's offset + 0x4B400000 where the search proved one, else
    0; the table carries that form if and only if every channel has one"""
    beta = host(f.constants("cuda")[1]).astype(np.int64)
    assert ((beta == 0) | (np.abs(beta - MAGIC) <= 127)).all(), beta
    return bool((beta != 0).all())


def _codes(w, x, store, N, H, W, inv, shift, fold, tab=True):
    _abi.set_option("first_tab", 1 if tab else 0)
    try:
        y, hp, wp = _abi.conv2d(w, x, store, 0, N, H, W, inv, shift, _abi.FN_QUANTIZED_TANH, 4, 2, _abi.STORE_I4, fold=fold)
    finally:
        _abi.set_option("first_tab", 1)
    tag = {_abi.STORE_U8: "mfma_i8_first_u8", _abi.STORE_F32_IMAGE: "mfma_i8_first_img255"}[store]
    assert _abi.last_kernel() == tag, _abi.last_kernel()
    return host(_abi.unpack(y, N * hp * wp, 64, _abi.STORE_I4, 4)).reshape(N, hp, wp, 64)


def _compare_all(layer, xu8, oracle=True):
    op, bn, w, inv, shift, f = layer
    N, H, W = xu8.shape[:3]
    x = (xu8.astype(F32) / F32(255)).astype(F32)
    want = O.maxpool2d(O.u8_conv_group(xu8, op, bn, Q(4)), 2) if oracle else None
    for xin, store in ((dev(xu8), _abi.STORE_U8), (dev(x), _abi.STORE_F32_IMAGE)):
        got = _codes(w, xin, store, N, H, W, inv, shift, f)
        pre = _codes(w, xin, store, N, H, W, inv, shift, f, tab=False)
        chain = _codes(w, xin, store, N, H, W, inv, shift, None)
        for name, ref in (("in-kernel preamble", pre), ("un-folded kernel", chain), ("oracle", want)):
            if ref is None:
                continue
            bad = np.argwhere(got != ref)
            assert bad.size == 0, "store %d against the %s: %d codes differ, first (n, y, x, c) = %s" % (
                store, name, len(bad), bad[0])
        assert len(np.unique(got)) >= 2                                  # not a saturated tensor
    w.check()                                                            # bytes / 255: inside the image domain


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("signs", ["pos", "neg", "mixed"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_table_and_bits_form_give_the_same_codes(shape, signs, bias):
    rng = np.random.default_rng(zlib.crc32(("%s %s %s" % (shape, signs, bias)).encode()))
    layer = _layer(rng, rng.uniform(-1, 1, (3, 3, 3, 64)), signs, bias)
    assert _table_has_bits(layer[5]), "no bits form after four draws: this case would test the fallback only"
    xu8 = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    _compare_all(layer, xu8, oracle=shape[0] <= 5)


@pytest.mark.parametrize("signs", ["pos", "mixed"])
def test_extreme_sums_of_saturated_filters(signs):
    """Images of all 0 and all 255 under filters whose 27 codes are all +7 (channels 0..15) or all -8 (16..31): both ends of
    those channels' domains, 0 and +-255 sum|k| with |sum k| = 189 and 216, are produced on the GPU -- the seeded accumulator
    furthest from 12582912, the fifteen-byte split of -sum k at its largest, and beta next to it."""
    rng = np.random.default_rng(99 + len(signs))
    k = rng.uniform(-1, 1, (27, 64))
    k[:, :16] = 0.875
    k[:, 16:32] = -1.0
    layer = _layer(rng, k.reshape(3, 3, 3, 64), signs, True)
    codes, _ = O.weight_codes(layer[0])
    assert (codes.reshape(27, 64)[:, :16] == 7).all() and (codes.reshape(27, 64)[:, 16:32] == -8).all()
    assert _table_has_bits(layer[5])
    for shape in ((3, 6, 16), (3, 32, 32)):
        xu8 = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
        xu8[0] = 0
        xu8[1] = 255
        _compare_all(layer, xu8)


@pytest.mark.parametrize("signs", ["pos", "mixed"])
def test_fallback_table_carries_the_mode3_constants(signs):
    """A handle whose bits search did not pass (forced: QNN_EPI_NO_FIRST_BITS at prepare) still has a table -- the preamble's
    own operands and the mode-3 constants -- and reports mode 3, usable."""
    kernel = np.random.default_rng(3).uniform(-1, 1, (3, 3, 3, 64))
    rng = np.random.default_rng(7 + len(signs))
    layer = _layer(rng, kernel, signs, True, bits=False)
    f = layer[5]
    assert f.mode == 3 and f.usable and not _table_has_bits(f)
    for shape in ((3, 32, 32), (2, 6, 16)):
        _compare_all(layer, rng.integers(0, 256, shape + (3,), dtype=np.uint8))
    # the same layer prepared with the bits search: the reported mode-3 constants are the same, only beta differs
    fb = _prepare(layer[2], layer[3], layer[4])
    np.testing.assert_array_equal(host(f.constants("cuda")[0]), host(fb.constants("cuda")[0]))
    assert (host(fb.constants("cuda")[1]) != 0).any() and (host(f.constants("cuda")[1]) == 0).all()


def test_float32_image_staging_still_raises_the_domain_flag():
    rng = np.random.default_rng(5)
    op, bn, w, inv, shift, f = _layer(rng, rng.uniform(-1, 1, (3, 3, 3, 64)), "mixed", True)
    assert _table_has_bits(f)
    N, H, W = 3, 32, 32
    xu8 = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    x = (xu8.astype(F32) / F32(255)).astype(F32)

    def raised():
        try:
            w.check()
        except _abi.QnnError as exc:
            assert "outside its domain" in str(exc)
            return True
        return False

    _codes(w, dev(x), _abi.STORE_F32_IMAGE, N, H, W, inv, shift, f)
    assert not raised()
    for i, val in enumerate((F32(0.5 / 255.0), F32("nan"), F32(1.01))):
        xb = x.copy()
        xb[i, 7 * i + 3, 15 + i, i] = val
        _codes(w, dev(xb), _abi.STORE_F32_IMAGE, N, H, W, inv, shift, f)
        assert raised(), val
        assert not raised()                                               # reported once, then cleared
