"""The oracle's convolutions (oracle.conv2d, oracle.int_conv2d) against an independent one: torch.nn.functional.conv2d in
float64 on the CPU, with TensorFlow's SAME padding applied explicitly by F.pad from the documented formula
(conv_geometry_cases.same_pads; nothing of the oracle's geometry is imported).  Inputs and weights are dyadic (codes / 8),
so every sum is exact and the comparison is equality, shape included.  No GPU.

tests/test_gpu_conv_geometry.py compares the kernels with the oracle on the same list; this file is what makes the
oracle a reference there for windows other than 3x3 and 1x1."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_geometry_cases as G
from oracle import qnn_oracle as O


def torch_conv(x, w, stride, padding):
    """NHWC x HWIO cross-correlation in float64."""
    kh, kw = w.shape[0], w.shape[1]
    xt = torch.as_tensor(np.asarray(x, dtype=np.float64)).permute(0, 3, 1, 2)
    wt = torch.as_tensor(np.asarray(w, dtype=np.float64)).permute(3, 2, 0, 1)
    if padding == "same":
        (pt, pb), (pl, pr) = G.same_pads(x.shape[1], kh, stride), G.same_pads(x.shape[2], kw, stride)
        xt = F.pad(xt, (pl, pr, pt, pb))
    return F.conv2d(xt, wt, stride=stride).permute(0, 2, 3, 1).numpy()


def _check(g, C=3, Cout=4):
    rng = np.random.default_rng(G.seed_of(g))
    xc = G.codes(rng, (2, g["H"], g["W"], C), -8, 7)
    wc = G.codes(rng, (g["kh"], g["kw"], C, Cout), -8, 7)
    st = (g["stride"], g["stride"])
    want = torch_conv(xc, wc, g["stride"], g["padding"])
    shape = (2, G.out_size(g["H"], g["kh"], g["stride"], g["padding"]), G.out_size(g["W"], g["kw"], g["stride"], g["padding"]), Cout)
    assert want.shape == shape, (G.geom_id(g), want.shape, shape)
    got_i = O.int_conv2d(xc, wc, st, g["padding"])
    assert got_i.shape == shape and np.array_equal(got_i.astype(np.float64), want), G.geom_id(g)
    got_f = O.conv2d((xc / 8.0).astype(np.float32), (wc / 8.0).astype(np.float32), st, g["padding"])
    assert got_f.dtype == np.float32 and got_f.shape == shape, G.geom_id(g)
    assert np.array_equal(got_f.astype(np.float64) * 64.0, want), G.geom_id(g)


def test_every_case_is_legal_and_every_category_is_present():
    assert len({G.geom_id(g) for g in G.GEOMS}) == len(G.GEOMS)
    seen = set()
    for g in G.GEOMS:
        assert G.legal(g), G.geom_id(g)
        assert g["H"] <= 12 and g["W"] <= 12
        seen |= G.categories(g)
    assert G.REQUIRED <= seen, sorted(G.REQUIRED - seen)
    # (5,5) and (5,6) sit on either side of the 32-bit tap mask of the tiled kernels (kh * kw + 3 <= 32)
    assert 5 * 5 + 3 <= 32 < 5 * 6 + 3
    assert [w for w in G.WINDOWS if G.packable(*w)] == [(1, 1), (1, 3), (3, 1), (2, 2), (2, 3), (3, 3)]


@pytest.mark.parametrize("window", G.WINDOWS, ids=lambda w: "%dx%d" % w)
def test_oracle_convolutions_equal_torch_float64_on_the_case_list(window):
    for g in G.GEOMS:
        if (g["kh"], g["kw"]) == window:
            _check(dict(g, pool=1))


def test_oracle_convolutions_equal_torch_float64_on_a_size_sweep():
    """Every window x stride x padding over heights 1..8 and widths 1, 2, 3, 5, 12: each legal combination."""
    n = 0
    for (kh, kw), s, pad, H, W in itertools.product(G.WINDOWS, G.STRIDES, G.PADDINGS, range(1, 9), (1, 2, 3, 5, 12)):
        g = dict(kh=kh, kw=kw, stride=s, padding=pad, H=H, W=W, pool=1)
        if G.legal(g):
            _check(g, C=2, Cout=3)
            n += 1
    assert n > 1800
