"""The EDGE staging of k_conv_mfma_halo (csrc/qnn_mfma_areg.hip): when an 8 x 2 tile spans the image width (16 x H images,
CIFAR B0) or a 4 x 4 tile is the image (8 x 8, CIFAR C0 and the conv + classifier form), a wave writes its LDS region's
padding once and then stages the image's pixels alone, as contiguous pieces of the image.
QNN_EPI_NO_HALO_EDGE = set_option("halo_edge", 0) keeps the general staging.

Every launch runs under the four combinations of halo_edge and fp6 (the un-folded float chain: under halo_edge alone) and
is compared, with no tolerance, with the default launch and with the oracle; the kernel tag is asserted.  BN scales are
mixed, all positive and all negative.  A batch larger than DISTINCT repeats DISTINCT images cyclically, among them
neighbours that are constant +7 and constant -8: a border the padding write missed, or one that a previous tile's pixels
reached, moves the sums by far more than a code step.
"""
import itertools
import zlib

import numpy as np
import pytest
import torch

import qnn_amd  # noqa: F401
from qnn_amd import _abi, engine, nets
from test_gpu_halo import CASES, _case
from test_gpu_halo_fp6 import _want
from test_gpu_halo_tab import DISTINCT, HALO, HEAD, SIGNS, _codes, _head, _layer, _Prepared, _want_head
from test_gpu_parity import BIN_ACT, Q, _oracle_group, _rand_bn, _run_group, dev, host

pytestmark = pytest.mark.gpu
F32 = np.float32
COMBOS = list(itertools.product((1, 0), (1, 0)))            # (halo_edge, fp6); the first is the default


class _Flags:
    def __init__(self, edge, fp6=1):
        self.v = (edge, fp6)

    def __enter__(self):
        _abi.set_option("halo_edge", self.v[0])
        _abi.set_option("fp6", self.v[1])

    def __exit__(self, *a):
        _abi.set_option("halo_edge", 1)
        _abi.set_option("fp6", 1)


def _conv(p, x):
    """the folded layer of a test_gpu_halo_tab._Prepared under every (halo_edge, fp6): [(codes, tag)]"""
    N, H, W, _ = x.shape
    xp = _abi.pack(dev(x), p.cin, _abi.FN_GRID, 4, _abi.STORE_I4)
    outs = []
    for edge, fp6 in COMBOS:
        with _Flags(edge, fp6):
            y, hp, wp = _abi.conv2d(p.w, xp, _abi.STORE_I4, 4, N, H, W, p.inv, p.shift, _abi.FN_QUANTIZED_TANH, 4, 2,
                                    _abi.STORE_I4, fold=p.f)
            outs.append((host(_abi.unpack(y, N * hp * wp, p.cout, _abi.STORE_I4, 4)).reshape(N, hp, wp, p.cout),
                         _abi.last_kernel()))
    return outs


def _conv_dense(p, x, dop, dbn):
    """conv + classifier in one launch under every (halo_edge, fp6): [(logits, tag)]"""
    N, H, W, _ = x.shape
    wd = engine._prepack(dop, _abi.STORE_I4, torch.device("cuda"))
    dinv, dshift = (dev(a) for a in engine.bn_constants(dbn))
    xp = _abi.pack(dev(x), 64, _abi.FN_GRID, 4, _abi.STORE_I4)
    outs = []
    for edge, fp6 in COMBOS:
        with _Flags(edge, fp6):
            y = _abi.conv2d_dense(p.w, wd, xp, _abi.STORE_I4, 4, N, H, W, p.inv, p.shift, _abi.FN_QUANTIZED_TANH, 4,
                                  dinv, dshift, fold=p.f)
            outs.append((host(y), _abi.last_kernel()))
    return outs


def _check(outs, want, tag):
    assert [k for _, k in outs] == [tag] * len(outs), [k for _, k in outs]
    for (got, _), combo in zip(outs, COMBOS):
        np.testing.assert_array_equal(got, outs[0][0], err_msg="(halo_edge, fp6) = %r against the default" % (combo,))
        np.testing.assert_array_equal(got, want, err_msg="(halo_edge, fp6) = %r against the oracle" % (combo,))


def _distinct(rng, h, w):
    """DISTINCT images; 3 / 4 and 8 / 9 are constant +7 / -8 neighbours, 5 has the two extremes on alternating rows"""
    xd = _codes(rng, (DISTINCT, h, w, 64))
    xd[3], xd[4], xd[8], xd[9] = 7 / 8, -1.0, -1.0, 7 / 8
    xd[5, ::2], xd[5, 1::2] = -1.0, 7 / 8
    return xd


def _waves(N, h, w):
    """(tiles, waves the launcher starts, waves per workgroup): halo_waves and launch_halo_one_f's grid, one filter slice"""
    twp = 8 if (w // 2) % 8 == 0 and (h // 2) % 2 == 0 else 4
    ntiles = N * ((w // 2) // twp) * ((h // 2) // (16 // twp))
    nw = 8 if ntiles >= 256 * 8 else 4
    return ntiles, min((ntiles + nw - 1) // nw, 256) * nw, nw


# ---- the B0 form: 8 x 2 tiles that span the width ----
@pytest.mark.parametrize("gamma_sign", SIGNS)
@pytest.mark.parametrize("shape", [(5, 16, 16, 64), (1, 16, 16, 64), (1, 4, 16, 64), (3, 8, 16, 64)],
                         ids=["n5", "n1", "one_tile", "two_tiles"])
def test_b0_form_small_batches(shape, gamma_sign):
    """four-wave workgroups, a wave per tile and fewer; (1, 4, 16): the rows above and below the tile are both padding"""
    rng = np.random.default_rng(zlib.crc32(("edge%r" % (shape,)).encode()))
    x = _codes(rng, shape)
    op, bn = _layer(rng, gamma_sign=gamma_sign)
    assert _waves(*shape[:3])[2] == 4
    _check(_conv(_Prepared(op, bn), x), _want(x, op, bn), HALO)


@pytest.mark.parametrize("gamma_sign", SIGNS)
@pytest.mark.parametrize("N,nw", [(300, 4), (600, 8)], ids=["four_waves", "eight_waves"])
def test_b0_form_waves_walk_on_to_other_images(N, nw, gamma_sign):
    """more tiles than waves: a wave's next tile lies in another image, whose borders must read as padding again"""
    ntiles, waves, got_nw = _waves(N, 16, 16)
    assert got_nw == nw and ntiles > waves, (ntiles, waves, got_nw)
    rng = np.random.default_rng(21 + N)
    xd = _distinct(rng, 16, 16)
    idx = np.arange(N) % DISTINCT
    op, bn = _layer(rng, gamma_sign=gamma_sign)
    _check(_conv(_Prepared(op, bn), xd[idx]), _want(xd, op, bn)[idx], HALO)


# ---- the C0 and classifier forms: the 4 x 4 tile is the image ----
@pytest.mark.parametrize("gamma_sign", SIGNS)
@pytest.mark.parametrize("N", [7, 1100], ids=["n7", "second_image_per_wave"])
def test_c0_form_conv(N, gamma_sign):
    ntiles, waves, nw = _waves(N, 8, 8)
    assert nw == 4 and (N == 7 or ntiles > waves), (ntiles, waves, nw)
    rng = np.random.default_rng(31 + N)
    xd = _distinct(rng, 8, 8)[:min(N, DISTINCT)]
    idx = np.arange(N) % len(xd)
    op, bn = _layer(rng, gamma_sign=gamma_sign)
    _check(_conv(_Prepared(op, bn), xd[idx]), _want(xd, op, bn)[idx], HALO)


@pytest.mark.parametrize("gamma_sign", SIGNS)
@pytest.mark.parametrize("N", [2048, 3], ids=["eight_waves", "four_waves"])
def test_conv_classifier(N, gamma_sign):
    rng = np.random.default_rng(41 + N)
    xd = _distinct(rng, 8, 8)[:min(N, DISTINCT)]
    idx = np.arange(N) % len(xd)
    op, bn = _layer(rng, gamma_sign=gamma_sign)
    dop, dbn = _head(rng)
    _check(_conv_dense(_Prepared(op, bn), xd[idx], dop, dbn), _want_head(xd, op, bn, dop, dbn)[idx], HEAD)


@pytest.mark.parametrize("xc", [-8, 7])
@pytest.mark.parametrize("wc", [-8, 7])
def test_extreme_codes_through_the_classifier_form(xc, wc):
    rng = np.random.default_rng(200 + 16 * xc + wc)
    x = np.full((3, 8, 8, 64), xc / 8, F32)
    x[1, :, ::3] = (-8 if xc == 7 else 7) / 8
    cw = np.full((3, 3, 64, 64), wc, F32)
    cw[..., 32:] = rng.choice([-8.0, 7.0], cw[..., 32:].shape)
    op, bn = _layer(rng, codes_w=cw)
    dop, dbn = _head(rng)
    _check(_conv_dense(_Prepared(op, bn), x, dop, dbn), _want_head(x, op, bn, dop, dbn), HEAD)


# ---- the padding pattern ----
@pytest.mark.parametrize("wc", [7, -8])
@pytest.mark.parametrize("shape", [(2, 16, 16, 64), (2, 8, 8, 64)], ids=["b0", "c0"])
def test_padding_pattern(shape, wc):
    """every input code -8 (staged as u = 0) against constant weights: a border left as it was found in LDS, or written
    as zero bits instead of u = 8, changes the sum of every edge position by a multiple of 64 * 8 * wc.  The BN is
    centred between the sums of the corner, edge and interior positions so that their codes differ."""
    rng = np.random.default_rng(51 + wc + shape[1])
    x = np.full(shape, -1.0, F32)
    op, bn = _layer(rng, codes_w=np.full((3, 3, 64, 64), wc, F32))
    sums = np.array([4, 6, 9], F32) * 64 * (-8 * wc) / 64          # conv values: 4 / 6 / 9 taps inside the image
    bn["mean"] = np.linspace(sums.min(), sums.max(), 64).astype(F32)
    bn["var"] = np.full(64, float(np.ptp(sums)) ** 2 / 4, F32)
    bn["beta"] = np.zeros(64, F32)
    want = _want(x, op, bn)
    assert len(np.unique(want)) > 2                                  # the positions do tell the paddings apart
    _check(_conv(_Prepared(op, bn, mode=None), x), want, HALO)


# ---- the un-folded forms (float chain; quantized and binary activations) share the staging ----
@pytest.mark.parametrize("name", ["b0", "c0", "one"])
def test_unfolded_forms(name):
    shape = dict((c[0], c[1]) for c in CASES)[name]
    rng, x, op = _case("edge" + name, shape, 64, bias=True)
    bn = _rand_bn(rng, 64, 9 * 64 * 0.12)
    for act in (Q(4), BIN_ACT):
        want = _oracle_group(x, op, bn, act, 2)
        for edge in (1, 0):
            with _Flags(edge):
                got, kern = _run_group(x, Q(4), op, bn, act, 2, _abi.STORE_I4)
            assert kern == HALO, kern
            np.testing.assert_array_equal(got, want, err_msg="halo_edge = %d" % edge)


# ---- geometries whose tiles do not span the image keep the general staging: the same codes under both values ----
@pytest.mark.parametrize("gamma_sign", SIGNS)
@pytest.mark.parametrize("name", ["wide", "big", "w24", "tall"])
def test_other_geometries_unchanged(name, gamma_sign):
    shape = dict((c[0], c[1]) for c in CASES)[name]
    rng = np.random.default_rng(zlib.crc32(("edge" + name).encode()))
    x = _codes(rng, shape)
    op, bn = _layer(rng, gamma_sign=gamma_sign)
    _check(_conv(_Prepared(op, bn), x), _want(x, op, bn), HALO)


# ---- whole networks ----
@pytest.mark.parametrize("net", [2, 1], ids=["headline", "bnn"])
def test_network_same_logits(net):
    cf = nets.baseline_config(net)
    spec = nets.build_spec(cf, nets.SEED_BASE + net)
    x = nets.synthetic_images(cf, 256, 5)
    outs = []
    for edge in (1, 0):
        with _Flags(edge):
            m = engine.FusedModel(spec, first_layer="exact")
            m.kernel_log = []
            outs.append(host(m(dev(x))))
            assert any("halo" in k for k in m.kernel_log), m.kernel_log
    np.testing.assert_array_equal(outs[0], outs[1])
