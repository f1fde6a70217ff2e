"""The byte first layer (csrc/qnn_first_u8.hip) after two changes that must not move a bit:

  * the pooled int4 forms DEAL their filters to the MFMA columns (column r of block nt = channel 4 r + nt), so a lane ends
    with four consecutive channels of a pooled pixel and the 8 x 8 nibble transpose across lanes is gone.  A wrong deal
    of the filter codes, of the negation for a negative BN scale, or of the A / B / fold tables puts a value into another
    channel's nibble: every case here uses per-channel distinct filters AND per-channel distinct, mixed-sign BN constants,
    on geometries that reach every strip / chunk / ragged-workgroup path of the launcher;
  * the float32 "image" staging keeps two running accumulators (an OR of the rounded bit patterns, a maximum of the
    rounding distances) and tests them once per kernel instead of clamping and comparing every element.  One off-grid
    value anywhere a lane stages -- either lane slot, either staged row, strip edges and halo columns, first and last
    row of a chunk -- must raise the layer's domain flag exactly as before, and exact bytes / 255 must not.

Reference: the specification of the typed image entry restated in oracle/qnn_oracle.py (u8_conv_group), bit-exact, as
tests/test_gpu_u8.py uses it.
"""
import itertools
import zlib

import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine
from oracle import qnn_oracle as O
from test_gpu_parity import BIN_ACT, Q, _rand_bn, dev, host

pytestmark = pytest.mark.gpu
F32 = np.float32


def _bank(rng, kind, which):
    """(3, 3, 3, 64) filters, every channel different from every other."""
    if which == "random":
        return rng.uniform(-1, 1, (3, 3, 3, 64)).astype(F32)
    c = np.arange(64)
    k = np.zeros((27, 64), F32)
    if kind == "binary":
        # +-1 only: one fixed sign pattern, with the six bits of the channel number written over the first six taps
        k[:] = np.where(rng.integers(0, 2, 27) > 0, 1.0, -1.0).astype(F32)[:, None]
        for b in range(6):
            k[b] = np.where((c >> b) & 1, 1.0, -1.0)
    else:
        # one-hot: channel c has its only weight on tap c % 27, with a magnitude / sign that depends on c // 27
        k[c % 27, c] = np.array([0.875, -1.0, 0.5], F32)[c // 27]
    assert len({k[:, j].tobytes() for j in range(64)}) == 64
    return k.reshape(3, 3, 3, 64)


def _mixed_bn(rng, scale):
    bn = _rand_bn(rng, 64, scale)
    sign = np.where((np.arange(64) * 7) % 5 < 2, -1.0, 1.0)           # irregular: differs inside every group of four
    bn["gamma"] = (np.abs(bn["gamma"]) * sign).astype(F32)
    return bn


# form -> (weight kind, weight bits, activation, folded)
FORMS = {"fold": ("quantized", 4, Q(4), True), "q4_chain": ("quantized", 4, Q(4), False),
         "q2_chain": ("quantized", 4, Q(2), False), "q3_chain": ("quantized", 3, Q(3), False),
         "bin": ("binary", None, BIN_ACT, False)}
# (N, H, W): W in {16, 32, 48} x H in {2, 6, 32} with an odd N, then: few tall images (the launcher splits an image's rows
# into chunks, nch > 1: also true of every H >= 8 above), task counts that leave the last workgroup of four waves ragged
# (5 x 1 x 1, 3 x 3 x 2 = 18, 3 x 3 x 1 = 9 tasks), and a single image
GEOMS = [(3, h, w) for w, h in itertools.product((16, 32, 48), (2, 6, 32))] + [(1, 66, 16), (5, 2, 16), (1, 32, 48), (7, 6, 32)]


def _run(w, x, store, N, H, W, inv, shift, act, fold):
    fn, ab = engine._act_code(act)
    y, hp, wp = _abi.conv2d(w, x, store, 0, N, H, W, inv, shift, fn, ab if fn == _abi.FN_QUANTIZED_TANH else 0, 2,
                            _abi.STORE_I4, fold=fold)
    kern = _abi.last_kernel()
    return host(_abi.unpack(y, N * hp * wp, 64, _abi.STORE_I4, ab if ab else 1)).reshape(N, hp, wp, 64), kern


@pytest.mark.parametrize("bank", ["distinct", "random"])
@pytest.mark.parametrize("geom", GEOMS, ids=["%dx%dx%d" % g for g in GEOMS])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_dealt_filters_give_the_specified_codes(form, geom, bank):
    kind, nb, act, folded = FORMS[form]
    N, H, W = geom
    rng = np.random.default_rng(zlib.crc32(("%s %s %s" % (form, geom, bank)).encode()))
    xu8 = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    op = {"op": "conv", "kind": kind, "kernel": _bank(rng, kind, bank), "strides": (1, 1), "padding": "same",
          "bias": (rng.standard_normal(64) * 0.05).astype(F32)}
    if nb:
        op["nb"] = nb
    # a one-hot filter's output is one byte / 255 times one weight: BN statistics of that size keep the codes spread
    bn = _mixed_bn(rng, 27 * 0.3 if bank == "random" or kind == "binary" else 0.08)
    want = O.maxpool2d(O.u8_conv_group(xu8, op, bn, act), 2)
    assert len(np.unique(want)) >= 2                                  # not a saturated tensor
    w = engine._prepack(op, _abi.STORE_F32, torch.device("cuda"), stride=1, same_pad=True)
    inv, shift = (dev(a) for a in engine.bn_constants(bn))
    f = None
    if folded:
        fn, ab = engine._act_code(act)
        f = _abi.Fold.try_prepare(w, _abi.STORE_U8, 0, inv, shift, fn, ab, _abi.STORE_I4)
        assert f is not None and f.mode == 3 and f.usable, (f and (f.mode, f.folded))     # the FOLD kernel form runs
    x = (xu8.astype(F32) / F32(255)).astype(F32)
    for xin, store, tag in ((dev(xu8), _abi.STORE_U8, "mfma_i8_first_u8"), (dev(x), _abi.STORE_F32_IMAGE, "mfma_i8_first_img255")):
        got, kern = _run(w, xin, store, N, H, W, inv, shift, act, f)
        assert kern == tag, kern
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s %s: %d codes differ, first (n, y, x, c) = %s" % (form, tag, len(bad), bad[0])
    w.check()                                                         # bytes / 255: inside the image domain


# ---------------------------------------------------------------------------------------------------------------
# staging of float32 images: the domain test on running accumulators
# ---------------------------------------------------------------------------------------------------------------
OFF_GRID = {"2^-14 above a byte": F32((100.0 + 2.0 ** -14) / 255.0), "2^-14 below a byte": F32((37.0 - 2.0 ** -14) / 255.0),
            "256/255": F32(256.0 / 255.0), "-1/255": F32(-1.0 / 255.0), "nan": F32("nan"), "+inf": F32("inf")}
# A strip of 16 conv columns stages input columns xs - 1 .. xs + 16 of two rows per step, 108 values: lane l takes value l
# (row 0 of the pair: columns up to xs + 16; lanes 54 .. 63: columns xs - 1 .. xs + 2 of row 1) and value l + 64 (the rest of
# row 1).  The pairs are (odd row, next even row).  Three 32 x 32 images are far fewer tasks than the persistent grid has
# waves, so the launcher's cost model cuts an image into its smallest chunks, two row pairs = four conv rows: every row
# 4 k is a chunk's first row and 4 k + 3 its last.  Columns 15 / 16 are the halo columns of strips 1 / 0 and the last / first own column of strips 0 / 1; columns
# 0 / 31 are a strip's first / last column next to the zero padding.
POSITIONS = [(0, 0, 0), (0, 15, 1), (0, 16, 2), (0, 31, 0),          # even row = row 1 of its pair; first row of chunk 0
              (3, 0, 1), (3, 2, 2), (3, 3, 0), (3, 15, 2), (3, 16, 0), (3, 31, 1),      # odd row = row 0; last row of chunk 0
              (4, 1, 0), (4, 3, 1), (4, 9, 2), (4, 16, 1), (4, 19, 0), (4, 20, 2),      # first row of chunk 1; both lane slots
              (7, 15, 0), (7, 17, 2), (28, 16, 1), (31, 0, 2), (31, 15, 1), (31, 31, 2)]


def _image_layer(cout=64, act=Q(4), fold=True):
    rng = np.random.default_rng(4242)
    op = {"op": "conv", "kind": "quantized", "nb": 4, "kernel": rng.uniform(-1, 1, (3, 3, 3, cout)).astype(F32),
          "bias": (rng.standard_normal(cout) * 0.05).astype(F32), "strides": (1, 1), "padding": "same"}
    bn = _mixed_bn(rng, 27 * 0.3) if cout == 64 else _rand_bn(rng, cout, 27 * 0.3)
    w = engine._prepack(op, _abi.STORE_F32, torch.device("cuda"), stride=1, same_pad=True)
    inv, shift = (dev(a) for a in engine.bn_constants(bn))
    fn, ab = engine._act_code(act)
    f = _abi.Fold.try_prepare(w, _abi.STORE_U8, 0, inv, shift, fn, ab, _abi.STORE_I4) if fold else None
    return op, bn, w, inv, shift, fn, ab, f


def _flag_raised(w):
    try:
        w.check()
    except _abi.QnnError as exc:
        assert "outside its domain" in str(exc)
        return True
    return False


def _every_byte_batch(N, H, W):
    xu8 = np.resize(np.arange(256, dtype=np.uint8), (N, H, W, 3)).astype(np.uint8)
    x = (xu8.astype(F32) / F32(255)).astype(F32)
    x[0, 1, 1, 1] = F32(-0.0)                                         # byte 0 written as -0.0: still the byte 0
    xu8[0, 1, 1, 1] = 0
    assert set(np.unique(xu8)) == set(range(256))
    return xu8, x


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "chain"])
def test_pooled_staging_flags_one_off_grid_value_wherever_it_is_staged(fold):
    op, bn, w, inv, shift, fn, ab, f = _image_layer(fold=fold)
    assert not fold or (f is not None and f.usable)
    N, H, W = 3, 32, 32
    xu8, x = _every_byte_batch(N, H, W)
    want = O.maxpool2d(O.u8_conv_group(xu8, op, bn, Q(4)), 2)

    def run(xv):
        y, hp, wp = _abi.conv2d(w, dev(xv), _abi.STORE_F32_IMAGE, 0, N, H, W, inv, shift, fn, ab, 2, _abi.STORE_I4, fold=f)
        assert _abi.last_kernel() == "mfma_i8_first_img255"
        return host(_abi.unpack(y, N * hp * wp, 64, _abi.STORE_I4, ab)).reshape(N, hp, wp, 64)

    # all 256 exact quotients k / 255 and -0.0: the specified codes, no flag
    np.testing.assert_array_equal(run(x), want)
    assert not _flag_raised(w)
    missed = []
    for name, val in OFF_GRID.items():
        for i, (yy, xx, c) in enumerate(POSITIONS):
            xb = x.copy()
            xb[i % N, yy, xx, c] = val
            run(xb)
            if not _flag_raised(w):
                missed.append((name, i % N, yy, xx, c))
            assert not _flag_raised(w)                                # reported once, then cleared
    assert not missed, missed
    np.testing.assert_array_equal(run(x), want)                       # and the accepted batch is accepted again
    assert not _flag_raised(w)


@pytest.mark.parametrize("cout,store", [(64, _abi.STORE_I4), (16, _abi.STORE_I4), (64, _abi.STORE_I8)],
                         ids=["c64_i4", "c16_i4", "c64_i8"])
def test_unpooled_staging_flags_the_same_values(cout, store):
    """k_conv_first_u8_full with float32 image input: the same staging, the same flag cases, one geometry."""
    act = Q(4) if store == _abi.STORE_I4 else Q(8)
    op, bn, w, inv, shift, fn, ab, _ = _image_layer(cout=cout, act=act, fold=False)
    N, H, W = 3, 32, 32
    xu8, x = _every_byte_batch(N, H, W)
    want = O.u8_conv_group(xu8, op, bn, act)

    def run(xv):
        y, ho, wo = _abi.conv2d(w, dev(xv), _abi.STORE_F32_IMAGE, 0, N, H, W, inv, shift, fn, ab, 1, store)
        assert _abi.last_kernel() == "mfma_i8_first_img255"
        return host(_abi.unpack(y, N * ho * wo, cout, store, ab)).reshape(N, ho, wo, cout)

    np.testing.assert_array_equal(run(x), want)
    assert not _flag_raised(w)
    missed = []
    for name, val in OFF_GRID.items():
        for i, (yy, xx, c) in enumerate(POSITIONS):
            xb = x.copy()
            xb[i % N, yy, xx, c] = val
            run(xb)
            if not _flag_raised(w):
                missed.append((name, i % N, yy, xx, c))
    assert not missed, missed
    np.testing.assert_array_equal(run(x), want)
    assert not _flag_raised(w)
