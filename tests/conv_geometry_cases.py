"""The window / stride / padding / image-size list of tests/test_conv_geometry_cpu.py (which proves the oracle's
convolution on it) and tests/test_gpu_conv_geometry.py (which runs the kernels on it).  Plain data and numpy: no test
in here, no GPU, nothing imported from the product or the oracle.

Every tensor is tiny (H, W <= 12) and every value dyadic, so each sum is exact in float32 in any order."""
import itertools

import numpy as np

F32 = np.float32

WINDOWS = ((1, 1), (1, 3), (3, 1), (2, 2), (2, 3), (3, 3), (4, 4), (3, 5), (5, 5), (5, 6), (7, 7))
STRIDES = (1, 2, 3)
PADDINGS = ("same", "valid")
# qnn_prepack_weights refuses a window with a side above 3 (QNN_EUNSUPPORTED), so no kernel is reachable on it: the GPU
# file runs the windows that fit and pins the refusal of the rest; the CPU file proves the oracle on all of them
PREPACK_MAX = 3


def packable(kh, kw):
    return kh <= PREPACK_MAX and kw <= PREPACK_MAX


def out_size(size, k, s, padding):
    """Output size of one axis by counting: VALID = window starts 0, s, 2s, ... whose window lies inside."""
    if padding == "same":
        return -(-size // s)
    return sum(1 for start in range(0, size, s) if start + k <= size)


def same_pads(size, k, s):
    """(before, after) of TensorFlow's SAME, as its documentation states it: the odd cell goes after."""
    total = max((out_size(size, k, s, "same") - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def stored_hw(g):
    return (out_size(g["H"], g["kh"], g["stride"], g["padding"]) // g["pool"],
            out_size(g["W"], g["kw"], g["stride"], g["padding"]) // g["pool"])


def legal(g):
    hp, wp = stored_hw(g)
    return hp > 0 and wp > 0


def _geom(kh, kw, stride, padding, H, W, pool=1):
    return dict(kh=kh, kw=kw, stride=stride, padding=padding, H=H, W=W, pool=pool)


def geom_id(g):
    return "%dx%d_s%d_%s_%dx%d%s" % (g["kh"], g["kw"], g["stride"], g["padding"], g["H"], g["W"],
                                     "_pool" if g["pool"] == 2 else "")


def _build():
    out = []
    for (kh, kw), s, pad in itertools.product(WINDOWS, STRIDES, PADDINGS):
        if pad == "same":
            # smaller than every window above 1x1 (each tap row partly outside); even H; odd H; W != H throughout
            sizes = [(2, 3), (6, 9), (7, 4)]
        else:
            # exactly the window (one output pixel); even H; odd H
            sizes = [(kh, kw), (max(kh, 6), max(kw, 9)), (max(kh, 7), max(kw, 4))]
        seen = []
        for H, W in sizes:
            if (H, W) not in seen:
                seen.append((H, W))
                out.append(_geom(kh, kw, s, pad, H, W))
    for kh, kw in WINDOWS:
        out.append(_geom(kh, kw, 1, "same", 5, 7, pool=2))           # pool behind an odd conv map: 5x7 -> 2x3
        out.append(_geom(kh, kw, 2, "same", 8, 12, pool=2))          # pool behind stride 2: 4x6 -> 2x3
        out.append(_geom(kh, kw, 2, "same", 7, 9, pool=2))           # ... and an odd map behind stride 2: 4x5 -> 2x2
    for kh, kw in ((1, 1), (2, 2), (2, 3), (3, 3)):
        out.append(_geom(kh, kw, 1, "valid", 7, 9, pool=2))          # VALID map (odd for 1x1, 2x3, 3x3), pooled
    return out


GEOMS = _build()


def categories(g):
    """The properties the list must keep covering (test_conv_geometry_cpu.py asserts each appears)."""
    kh, kw, s, pad, H, W = g["kh"], g["kw"], g["stride"], g["padding"], g["H"], g["W"]
    ho, wo = out_size(H, kh, s, pad), out_size(W, kw, s, pad)
    c = {"window_%dx%d" % (kh, kw), "stride_%d" % s, pad, "%s_h_stride_%d" % ("even" if H % 2 == 0 else "odd", s)}
    if pad == "same" and H < kh and W < kw:
        c.add("same_image_smaller_than_window")
    if pad == "valid" and (H, W) == (kh, kw):
        c.add("valid_image_is_the_window")
    if W != H:
        c.add("w_differs_from_h")
    if s > max(kh, kw):
        c.add("stride_above_window")
    if kh != kw:
        c.add("rectangular")
    if pad == "same" and (same_pads(H, kh, s)[0] != same_pads(H, kh, s)[1] or same_pads(W, kw, s)[0] != same_pads(W, kw, s)[1]):
        c.add("same_pads_more_after")
    if g["pool"] == 2:
        c.add("pool")
        if ho % 2 or wo % 2:
            c.add("pool_behind_odd_map")
        if s == 2:
            c.add("pool_behind_stride_2")
    return c


REQUIRED = ({"window_%dx%d" % w for w in WINDOWS} | {"stride_%d" % s for s in STRIDES} | set(PADDINGS) |
            {"%s_h_stride_%d" % (p, s) for p in ("even", "odd") for s in STRIDES} |
            {"same_image_smaller_than_window", "valid_image_is_the_window", "w_differs_from_h", "stride_above_window",
             "rectangular", "same_pads_more_after", "pool", "pool_behind_odd_map", "pool_behind_stride_2"})


def codes(rng, shape, lo, hi):
    """Integer codes in [lo, hi] as int64."""
    return rng.integers(lo, hi + 1, size=shape).astype(np.int64)


def seed_of(g, salt=0):
    return (((g["kh"] * 8 + g["kw"]) * 4 + g["stride"]) * 2 + (g["padding"] == "same")) * 4096 + g["H"] * 64 + g["W"] * 4 + \
        g["pool"] + 1000003 * salt
