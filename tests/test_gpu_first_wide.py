"""The byte first layer's image-wide strip (csrc/qnn_first_u8.hip, SW = 32): W = 32 is walked as one strip per image, three
staged values per lane, no column halo, four tiles and two packing epilogues per step.

Every launch is compared, bit for bit, with the same call under QNN_EPI_NO_FIRST_WIDE (set_option("first_wide", 0): the
two 16-column strips) and with the oracle's restatement of the typed entry (oracle/qnn_oracle.py, u8_conv_group), through
both entries (uint8 bytes and float32 bytes / 255).  The kernel log's name is the route's and does not tell the two forms
apart, so the comparison with the off switch is what shows that both ran the same arithmetic.

Shapes: one step; two steps; an odd number of steps with more than one image; the benchmark's height; one tall image whose
column the planner cuts into chunks.  (A batch beyond the resident waves is not here: with a grid capped by the task count
`task += nw` runs no differently at (2, 32) than at any batch the other files already run.)
"""
import zlib

import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine, nets
from oracle import qnn_oracle as O
from test_gpu_parity import BIN_ACT, Q, _rand_bn, dev, host

pytestmark = pytest.mark.gpu
F32 = np.float32
TAG = {_abi.STORE_U8: "mfma_i8_first_u8", _abi.STORE_F32_IMAGE: "mfma_i8_first_img255"}
SHAPES = [(1, 2), (1, 4), (3, 6), (5, 32), (1, 96)]


def plan(N, rows, cap=1024, fill=1.5):
    """qnn_strip_plan(N, 1, rows, cap, 1.5, 2) restated: (rc, nch)."""
    best = None
    for rc in range(2, rows + 2, 2):
        nch = -(-rows // rc)
        cost = -(-(N * nch) // (4 * cap)) * (rc + fill)
        if best is None or cost < best[0]:
            best = (cost, rc, nch)
    return best[1], best[2]


def test_the_tall_image_is_cut_into_chunks():
    rc, nch = plan(1, 48)
    assert nch > 1 and rc % 2 == 0, (rc, nch)
    assert plan(5, 16)[1] > 1 and plan(1, 1) == (2, 1)                    # (5, 32) is chunked too; (1, 2) is one step


def images(rng, N, H):
    """Random bytes with 0 and 255 on the image's border columns and rows and on both sides of every tile border."""
    x = rng.integers(0, 256, (N, H, 32, 3), dtype=np.uint8)
    for c, v in ((0, 0), (31, 255), (7, 255), (8, 0), (15, 0), (16, 255), (23, 255), (24, 0)):
        x[:, ::2, c] = v
        x[:, 1::2, c] = 255 - v
    x[:, 0, 1:31:3] = 0
    x[:, 0, 2:31:3] = 255
    x[:, H - 1, 1:31:3] = 255
    x[:, H - 1, 2:31:3] = 0
    return x


def layer(seed, nb=4, extreme=False):
    rng = np.random.default_rng(seed)
    k = rng.uniform(-1, 1, (3, 3, 3, 64))
    if extreme:                                                          # codes -2^(nb-1) and 2^(nb-1) - 1, whole filters
        k[..., :8] = -1.0
        k[..., 8:16] = 1.0
    op = {"op": "conv", "kind": "quantized", "nb": nb, "kernel": k.astype(F32), "strides": (1, 1), "padding": "same",
          "bias": (rng.standard_normal(64) * 0.05).astype(F32)}
    bn = _rand_bn(rng, 64, 27 * 0.3)
    g = np.abs(bn["gamma"]) * np.where((np.arange(64) * 7) % 5 < 2, -1.0, 1.0)   # mixed signs inside every group of four
    bn["gamma"] = g.astype(F32)
    w = engine._prepack(op, _abi.STORE_F32, torch.device("cuda"), stride=1, same_pad=True)
    inv, shift = (dev(a) for a in engine.bn_constants(bn))
    return op, bn, w, inv, shift


def fold_of(w, inv, shift, bits):
    _abi.set_option("first_bits", 1 if bits else 0)
    try:
        f = _abi.Fold.try_prepare(w, _abi.STORE_U8, 0, inv, shift, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4)
    finally:
        _abi.set_option("first_bits", 1)
    assert f is not None and f.mode == 3 and f.usable
    return f


def run(w, x, store, inv, shift, fn, ab, pool, out_store, fold=None, wide=True, tab=True):
    N, H, W = x.shape[:3]
    _abi.set_option("first_wide", 1 if wide else 0)
    _abi.set_option("first_tab", 1 if tab else 0)
    try:
        y, hp, wp = _abi.conv2d(w, x, store, 0, N, H, W, inv, shift, fn, ab, pool, out_store, fold=fold)
    finally:
        _abi.set_option("first_wide", 1)
        _abi.set_option("first_tab", 1)
    assert _abi.last_kernel() == TAG[store], _abi.last_kernel()
    if out_store == _abi.STORE_F32:
        return host(y)
    return host(_abi.unpack(y, N * hp * wp, 64, out_store, ab if ab else 1)).reshape(N, hp, wp, 64)


def both_entries(xu8):
    x = (xu8.astype(F32) / F32(255)).astype(F32)
    return ((dev(xu8), _abi.STORE_U8), (dev(x), _abi.STORE_F32_IMAGE))


def same(got, ref, what):
    bad = np.argwhere(got != ref)
    assert bad.size == 0, "%s: %d values differ, first (n, y, x, c) = %s" % (what, len(bad), bad[0])


# form: (fold: None | "bits" | "mode3", first_tab, activation, pool, output store)
FORMS = {"fold_bits": ("bits", True, Q(4), 2, _abi.STORE_I4), "fold_mode3": ("mode3", True, Q(4), 2, _abi.STORE_I4),
         "fold_notab": ("bits", False, Q(4), 2, _abi.STORE_I4), "chain": (None, True, Q(4), 2, _abi.STORE_I4),
         "bin": (None, True, BIN_ACT, 2, _abi.STORE_I4), "f32_none": (None, True, None, 1, _abi.STORE_F32)}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_wide_strip_gives_the_narrow_strips_bits_and_the_oracles(shape, form):
    N, H = shape
    fold, tab, act, pool, out_store = FORMS[form]
    seed = zlib.crc32(("%s %s" % (shape, form)).encode())
    op, bn, w, inv, shift = layer(seed)
    f = fold_of(w, inv, shift, fold == "bits") if fold else None
    fn, ab = engine._act_code(act) if act else (_abi.FN_NONE, 0)
    ab = ab if fn == _abi.FN_QUANTIZED_TANH else 0
    xu8 = images(np.random.default_rng(seed + 1), N, H)
    want = O.u8_conv_group(xu8, op, bn, act)
    want = O.maxpool2d(want, 2) if pool == 2 else want
    for x, store in both_entries(xu8):
        got = run(w, x, store, inv, shift, fn, ab, pool, out_store, f, tab=tab)
        narrow = run(w, x, store, inv, shift, fn, ab, pool, out_store, f, wide=False, tab=tab)
        same(got, narrow, "store %d, wide against the 16-column strips" % store)
        same(got, want.astype(F32), "store %d, wide against the oracle" % store)
        assert len(np.unique(got)) >= 2
    w.check()


def test_weight_codes_at_the_ends_the_route_admits():
    """7-bit weights (wshift 6): whole filters of code -64, and +64 where a negative BN scale negates them."""
    op, bn, w, inv, shift = layer(77, nb=7, extreme=True)
    codes, ws = O.weight_codes(op)
    assert ws == 6 and (codes[..., :8] == -64).all() and (codes[..., 8:16] == 63).all()
    assert (bn["gamma"][:8] < 0).any() and (bn["gamma"][:8] > 0).any()
    xu8 = images(np.random.default_rng(78), 3, 6)
    xu8[1] = 255
    xu8[2] = 0
    want = O.maxpool2d(O.u8_conv_group(xu8, op, bn, Q(4)), 2).astype(F32)
    for x, store in both_entries(xu8):
        got = run(w, x, store, inv, shift, _abi.FN_QUANTIZED_TANH, 4, 2, _abi.STORE_I4)
        same(got, run(w, x, store, inv, shift, _abi.FN_QUANTIZED_TANH, 4, 2, _abi.STORE_I4, wide=False), "narrow")
        same(got, want, "oracle")


def test_every_staged_lane_slot_raises_the_domain_flag():
    """bytes / 255 except one element, at the image's two corners and at one position for each of a lane's three staged
    elements (lane 40 of the row pair (1, 2): flat indices 40, 104, 168 of its 192 values = (row 1, col 13, ch 1), (row 2,
    col 2, ch 2), (row 2, col 24, ch 0)); the clean batch leaves the flag clear and gives the uint8 entry's bits."""
    op, bn, w, inv, shift = layer(5)
    f = fold_of(w, inv, shift, True)
    N, H = 2, 6
    xu8 = images(np.random.default_rng(6), N, H)
    x = (xu8.astype(F32) / F32(255)).astype(F32)
    args = (inv, shift, _abi.FN_QUANTIZED_TANH, 4, 2, _abi.STORE_I4, f)

    def raised():
        try:
            w.check()
        except _abi.QnnError as exc:
            assert "outside its domain" in str(exc)
            return True
        return False

    clean = run(w, dev(x), _abi.STORE_F32_IMAGE, *args)
    assert not raised()
    same(clean, run(w, dev(xu8), _abi.STORE_U8, *args), "float32 image entry against the uint8 entry")
    places = [(0, 0, 0), (H - 1, 31, 2), (1, 13, 1), (2, 2, 2), (2, 24, 0)]
    for row, col, ch in places:
        half = F32((float(xu8[1, row, col, ch]) + 0.5) / 255.0)             # 0.5 / 255 off its byte
        for val in (half, F32(-1.0 / 255.0), F32(256.0 / 255.0), F32("nan")):
            xb = x.copy()
            xb[1, row, col, ch] = val
            run(w, dev(xb), _abi.STORE_F32_IMAGE, *args)
            assert raised(), (row, col, ch, val)
            assert not raised()


@pytest.mark.parametrize("W", [16, 48, 64])
def test_other_widths_keep_the_narrow_strips(W):
    op, bn, w, inv, shift = layer(100 + W)
    f = fold_of(w, inv, shift, True)
    xu8 = np.random.default_rng(W).integers(0, 256, (3, 6, W, 3), dtype=np.uint8)
    want = O.maxpool2d(O.u8_conv_group(xu8, op, bn, Q(4)), 2).astype(F32)
    for x, store in both_entries(xu8):
        got = run(w, x, store, inv, shift, _abi.FN_QUANTIZED_TANH, 4, 2, _abi.STORE_I4, f)
        same(got, want, "W = %d against the oracle" % W)
        same(got, run(w, x, store, inv, shift, _abi.FN_QUANTIZED_TANH, 4, 2, _abi.STORE_I4, f, wide=False), "switch")


def test_headline_model_logits_do_not_move():
    cf = nets.baseline_config(2)
    spec = nets.build_spec(cf, nets.SEED_BASE + 2)[:-1]
    m = engine.FusedModel(spec)
    xu8 = nets.synthetic_images_u8(cf, 8, 3)
    x = dev((xu8.astype(F32) / F32(255)).astype(F32))
    m.kernel_log = []
    y1 = host(m(x)).copy()
    assert m.kernel_log[0] == TAG[_abi.STORE_F32_IMAGE], m.kernel_log[:3]
    _abi.set_option("first_wide", 0)
    try:
        y0 = host(m(x)).copy()
    finally:
        _abi.set_option("first_wide", 1)
    np.testing.assert_array_equal(y1, y0)
    np.testing.assert_array_equal(y1, O.run_spec_u8(spec, xu8))
