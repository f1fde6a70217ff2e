"""quantized_relu / quantized_leakyrelu as fused conv epilogues on their special points, kernel by kernel: the tensors,
shortcut planting and case dicts of epilogue_grid_cases.py with the two functions of qrelu_cases.py (held bit for bit to
golden/ref_qrelu.npz by test_qrelu_cpu.py) as the activation.  A plain module: test_qact_grid_cpu.py proves what every
case carries, test_gpu_qact_grid.py runs the cases.

The points (m = 2^(nb-1)):
  quantized_relu       code = clamp(rint(fadd_rn(v, 1) * m) - m, 0, m - 1).  Ties (k + 1/2) / m inside the clip range; the lower
                       edge region v = +-1 / (2m), 0, -1 / m; the upper edge (m - 1) / m and (m - 1/2) / m; exact zeros.
                       With a float32 shortcut also both float32 neighbours of the ties: v + 1 rounds a neighbour ONTO the
                       tie, so half-to-even decides its code, and a chain without that rounding, clamp(rint(v * m), 0, m - 1),
                       gives another code below an odd k and above an even k.
  quantized_leakyrelu  w = v for v >= 0, fmul_rn(0.1f, v) below; code = clamp(rint(w * m), -m, m - 1).  The positive ties; the
                       negative ties v = -(10k + 5) / m, dyadic inputs whose ROUNDED product is exactly -(k + 1/2) / m while
                       the exact product float32(0.1) * v lies just beyond it (a chain that rounds once differs for even k);
                       exact zeros; the upper clip edge.  With a float32 shortcut also the float32 neighbours of the
                       negative ties.
NOT covered here: the lower clip edge of quantized_leakyrelu needs v <= -10, which these layers do not reach -- the
elementwise vectors of ref_qrelu.npz cover it.  And the negative ties of Q(2) are the single input v = -2.5, which these
layers reach only where a float32 shortcut (values down to -4) carries them there: a packed shortcut is >= -1, and four
of 25600 outputs of the widest layer land on it by themselves.  So the Q(2) negative ties are claimed by the float32-
shortcut cases only (claims_negative()); those of Q(4) and Q(8), from -5/8 and -5/128 on, by every case.  The CPU test
prints every count, claimed or not.  Clip edges are claimed as claims_edges() says.

Behind the conv table: the in-launch projection form and the dense kernels (proj_cases, DENSE)."""
import numpy as np

import epilogue_grid_cases as G
import qrelu_cases as Q

F32 = np.float32
RELU, LEAKY = Q.FNS
MIN_TIES, MIN_ZEROS, MIN_EDGE, MIN_DIFF = G.MIN_TIES, G.MIN_ZEROS, G.MIN_EDGE, G.MIN_DIFF


def _nbr(t):
    """(float32 below, float32 above) of a dyadic t, as Python floats."""
    t = F32(t)
    return float(np.nextafter(t, F32(-np.inf))), float(np.nextafter(t, F32(np.inf)))


def pos_ties(nb):
    """The ties (k + 1/2) / m with both neighbouring codes inside [0, m - 1]; at most the eight nearest to zero."""
    m = 2 ** (nb - 1)
    return [(k + 0.5) / m for k in range(min(m - 1, 8))]


def neg_ties(nb):
    """v = -(10k + 5) / m with v > -4 (what a shortcut can reach): 0.1f * v rounds to -(k + 1/2) / m exactly."""
    m = 2 ** (nb - 1)
    out = [-(10 * k + 5) / m for k in range(8) if (10 * k + 5) / m < 4 and k + 0.5 < m]
    for v in out:
        w = float(Q.ALPHA * F32(v)) * m
        assert w - np.floor(w) == 0.5 and float(Q.ALPHA) * v * m < w, (nb, v)          # the exact product lies beyond the tie
    return out


def _plant(fn, nb):
    m = 2 ** (nb - 1)
    edges = [0.0, (m - 1) / m, (m - 0.5) / m]
    if fn == RELU:
        dy = pos_ties(nb) + edges + [-0.5 / m, -1.0 / m]
        f32 = [x for t in pos_ties(nb) for x in _nbr(t)]
    else:
        dy = pos_ties(nb)[:4] + neg_ties(nb) + edges
        f32 = [x for t in neg_ties(nb) for x in _nbr(t)]
    return tuple((t, 32) for t in dy) + tuple((t, 16, "f32") for t in f32)


PLANT = {(fn, nb): _plant(fn, nb) for fn in Q.FNS for nb in (2, 4, 8)}          # every case carries it as c["plant"]


# ---------------------------------------------------------------------------------------------------------------------
# what a case carries, counted on the oracle's pre-activation p
# ---------------------------------------------------------------------------------------------------------------------
def _frac_half(t):
    return t - np.floor(t) == 0.5


def tie_count(p, nb):
    """Positive ties: p * m a half-integer strictly between the codes 0 and m - 1 (both functions)."""
    m = 2.0 ** (nb - 1)
    t = p.astype(np.float64) * m
    return int(np.count_nonzero(_frac_half(t) & (t > 0) & (t < m - 1)))


def neg_tie_count(p, nb):
    """quantized_leakyrelu: p < 0 whose rounded product 0.1f * p is a tie inside the clip range."""
    m = 2.0 ** (nb - 1)
    w = (Q.ALPHA * p).astype(F32).astype(np.float64) * m
    return int(np.count_nonzero((p < 0) & _frac_half(w) & (w > -m)))


def zero_count(p):
    return int(np.count_nonzero(p == 0))


def edge_counts(p, fn, nb):
    """(points of the lower edge region +-1 / (2m), 0, -1 / m -- quantized_relu; None for quantized_leakyrelu --, points of
    the upper edge (m - 1) / m, (m - 1/2) / m).  A region counts as 0 where one of its values does not occur at all."""
    m = 2.0 ** (nb - 1)
    t = p.astype(np.float64) * m

    def region(values):
        n = [int(np.count_nonzero(t == x)) for x in values]
        return sum(n) if min(n) else 0
    hi = region((m - 1, m - 0.5))
    if fn == LEAKY:
        return None, hi
    return region((-1.0, -0.5, 0.0, 0.5)), hi


def _value(c, code, lo, nb):
    m = 2.0 ** (nb - 1)
    return G._pool(c, (np.clip(code, lo, m - 1) / m).astype(F32))


def _t(p, fn, nb):
    """(float64 code-unit value behind the contract's one rounding, offset, lower clip)."""
    m = 2.0 ** (nb - 1)
    if fn == RELU:
        return (p + F32(1)).astype(F32).astype(np.float64) * m, m, 0.0
    return np.where(p >= 0, p, (Q.ALPHA * p).astype(F32)).astype(np.float64) * m, 0.0, -m


def wrong_half_away(c, p, fn, nb):
    """The contract with ties rounded away from zero."""
    t, off, lo = _t(p, fn, nb)
    return _value(c, np.sign(t) * np.floor(np.abs(t) + 0.5) - off, lo, nb)


def wrong_floor_half(c, p, fn, nb):
    """The contract with floor(x + 0.5): ties rounded up."""
    t, off, lo = _t(p, fn, nb)
    return _value(c, np.floor(t + 0.5) - off, lo, nb)


def wrong_one_rounding(c, p, fn, nb):
    """quantized_relu without the v + 1 rounding, clamp(rint(v * m), 0, m - 1); quantized_leakyrelu with one rounding, rint
    of the float64 product float32(0.1) * v * m.  Both in float64."""
    m = 2.0 ** (nb - 1)
    p64 = p.astype(np.float64)
    if fn == RELU:
        return _value(c, np.rint(p64 * m), 0.0, nb)
    return _value(c, np.rint(np.where(p64 >= 0, p64, float(Q.ALPHA) * p64) * m), -m, nb)


def kinds(c):
    return sorted({(a["fn"], a["nb"]) for a in c["acts"]})


def claims_edges(c):
    """Clip edges are claimed where the grid reaches them by itself (no BN) or a shortcut plants them: a float32 one, or a
    packed one at post_scale 1 (codes end at 7/8: scaled by 1/2 or 1/4 the merge reaches (m - 1/2) / m only from a
    pre-residual value the dyadic BN hardly ever gives)."""
    return c["epi"] == "nobn" or c["res"] == SF32 or (c["res"] is not None and c["post_scale"] == 1.0)


def claims_negative(c, nb):
    """The dyadic negative ties of quantized_leakyrelu start at -5 / m: -5/128 and -5/8 lie inside every layer's range and are
    claimed by every case, -2.5 (Q(2)) only where a float32 shortcut plants it (module docstring)."""
    return nb != 2 or c["res"] == SF32


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
def _acts(pairs, named=True):
    return [G.A(fn, nb, store, named) for fn in Q.FNS for nb, store in pairs]


I4, I8, SF32 = G.STORE_I4, G.STORE_I8, G.STORE_F32
ACTS_I4 = _acts([(4, I4), (2, I4)])
ACTS_GEN = _acts([(4, I4), (2, I4), (4, SF32)])
ACTS_GEN8 = _acts([(4, I4), (2, I4), (8, I8), (4, SF32)])
ACTS_I8 = _acts([(8, I8)])
ACTS_F32 = _acts([(4, SF32)])


def _table():
    t = []

    def case(*a, **kw):
        return dict(G._case(*a, **kw), plant=PLANT)
    # ---- the un-folded int4 strip kernels; the twin of every case is k_conv_generic under QNN_EPI_NO_STRIP.
    # 10 rows = chunks of 4, 4 and 2, 20 columns = a whole and a ragged strip
    for C in (16, 32, 64):
        name, shape = "strip_i4_c%d" % C, (2, 10, 20, C)
        t.append(case(name, "generic", I4, shape, C, ACTS_I4))
        t.append(case(name, "generic", I4, shape, C, ACTS_I4, bias=False))
        # (16 channels behind the dyadic BN: four images, as two hold 18 and 27 times the one tie of Q(2), v = 1/4)
        bn_shape = (4, 10, 20, C) if C == 16 else shape
        t.append(case(name, "generic", I4, bn_shape, C, ACTS_I4, "dyadic", "mixed"))
        t.append(case(name, "generic", I4, bn_shape, C, ACTS_I4, "dyadic", "neg"))
        for post in (1.0, 0.5, 0.25):
            # (at 1/4 behind the "wide" BN: the negative tie -5/8 needs a pre-residual value <= -1.5 there, which the other
            # dyadic BNs give the 16-channel layer twice in two images)
            t.append(case(name, "generic", I4, shape, C, ACTS_I4, "residual", "mixed" if post != 0.25 else "wide", I4, 4, post))
        t.append(case(name, "generic", I4, shape, C, ACTS_I4, "residual", None, I4, 2, 1.0))
        t.append(case(name, "generic", I4, shape, C, ACTS_I4, "residual", "mixed", SF32, 0, 1.0))
        t.append(case(name, "generic", I4, shape, C, ACTS_I4, "residual", None, SF32, 0, 0.5))
    for C in (16, 32):
        name, shape = "strip_i4_c%d_s2" % C, (2, 19, 21, C)
        t.append(case(name, "generic", I4, shape, 2 * C, ACTS_I4, stride=2))
        # (16 channels: four images, for the 32 ties of Q(2) again)
        t.append(case(name, "generic", I4, (4, 19, 21, C) if C == 16 else shape, 2 * C, ACTS_I4, "dyadic", "mixed", stride=2))
    # ---- k_conv_generic: 24 channels (no matrix-pipe kernel takes them), every output store
    shape = (2, 10, 20, 24)
    t.append(case("generic", "generic", I4, shape, 24, ACTS_GEN))
    t.append(case("generic", "generic", I4, shape, 24, ACTS_GEN8, "dyadic", "mixed"))
    t.append(case("generic", "generic", I4, shape, 24, ACTS_GEN, "residual", "mixed", I4, 4, 0.5))
    t.append(case("generic", "generic", I4, shape, 24, ACTS_GEN8, "residual", "mixed", SF32, 0, 1.0))
    # pooled, int8 operands: where the pooled VGG layers of these networks run.  Q(8), the width of those layers: behind
    # the pool a Q(4) negative tie (-5/8) would have to be the largest value of its window
    for sign in ("neg", "mixed"):
        # (four images: two hold 17 and 25 exact zeros)
        t.append(case("generic", "generic", I8, (4, 10, 20, 24), 24, ACTS_I8, "dyadic", sign, pool=2))
        t[-1]["id"] += "-xi8"
    # float32 values in, float32 out
    for c in (case("generic", "generic", SF32, shape, 24, ACTS_F32), case("generic", "generic", SF32, shape, 24, ACTS_F32, "dyadic", "mixed")):
        c["id"] += "-xf32"
        t.append(c)
    # dilated (d = 2), pinned to k_conv_generic by the channel count
    t.append(case("generic", "generic", I4, shape, 24, ACTS_GEN, d=2))
    t.append(case("generic", "generic", I4, (4, 10, 20, 24), 24, ACTS_GEN, "dyadic", "mixed", d=2))       # (four images: Q(2) ties)
    assert len({c["id"] for c in t}) == len(t)
    return t


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _table()
    return _CASES


# ---------------------------------------------------------------------------------------------------------------------
# the in-launch projection form: the shortcut is the 1x1 strides-2 convolution of a block input with half the channels,
# computed inside the launch, so nothing can be planted -- a case carries whatever the grid yields, and the CPU test
# states the counts.  The twin is the two-launch form (the projection as a float32 tensor, then res_store = F32).
# ---------------------------------------------------------------------------------------------------------------------
def proj_cases():
    out = []
    for C in (32, 64):
        for sign in (None, "mixed"):
            N = 2 if sign is None else 6      # (behind the BN six images: two of the 32-channel layer hold 28 Q(2) ties and 5 negative ones, four hold 7)
            main = G._case("strip_i4_c%d" % C, "generic", I4, (N, 10, 20, C), C, ACTS_I4, "nobn" if sign is None else "dyadic", sign)
            out.append(dict(id=main["id"] + "-proj", main=main, acts=ACTS_I4, pool=1, post_scale=0.5,
                            pbase=(I4, N, 19, 40, C // 2, C, 1, 2, True)))         # 19 x 40 -> 10 x 20 at strides 2
    return out


def proj_preactivation(pc):
    v, r = G.pre_residual(pc["main"]), G.base(*pc["pbase"])["conv"]
    assert r.shape == v.shape
    return ((r + v).astype(F32) * F32(pc["post_scale"])).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# dense layers with the function as the epilogue fn (nb 4), float32 out: k_dense_packed (more than 16 units, and up to 16
# units where the split form does not apply), k_dense_packed_split (up to 16 units AND a row of a multiple of 16 words,
# K = 128 at 4 bits -- K = 64 and 96 do not reach it) and k_dense_f32in.  qnn_last_kernel says dense_i4 for both packed
# forms; the shape decides between them (launch_dense, csrc/qnn_conv.hip).
# ---------------------------------------------------------------------------------------------------------------------
DENSE_ROWS = 512
DENSE = [dict(id="dense_packed-k%d-u%d" % (K, U), kernel="dense_i4", form="packed", K=K, units=U, x_store=I4)
         for K, U in ((64, 32), (96, 32), (96, 10))] + \
        [dict(id="dense_split-k128-u10", kernel="dense_i4", form="split", K=128, units=10, x_store=I4)] + \
        [dict(id="dense_f32-k%d-u%d" % (K, U), kernel="dense_f32", form="f32", K=K, units=U, x_store=SF32) for K, U in ((64, 32), (96, 10))]
_DENSE = {}


def dense_layer(dc):
    """(x, dense op, inv, shift, pre-activation) of a dense case: 4-bit grid values against weight codes -2 .. 2, a bias and
    a shift in multiples of 2^-4, a power-of-two inv of either sign in 1/2 .. 4 -- every value a small dyadic number."""
    if dc["id"] not in _DENSE:
        from oracle import qnn_oracle as O
        K, U = dc["K"], dc["units"]
        rng = np.random.default_rng(G._seed("dense", K, U, dc["x_store"]))
        x = (np.clip(np.rint(rng.standard_normal((DENSE_ROWS, K)) * 2), -8, 7) / 8.0).astype(F32)
        op = {"op": "dense", "kind": "quantized", "nb": 4, "kernel": (rng.integers(-2, 3, (K, U)) / 8.0).astype(F32),
              "bias": (rng.integers(-4, 5, U) / 16.0).astype(F32)}
        u = np.arange(U)
        inv = np.array([1.0, -1.0, 0.5, 2.0, -2.0, 1.0, 4.0, -0.5])[u % 8].astype(F32)
        shift = (((u % 5) - 2) / 16.0).astype(F32)
        v = O.quantized_dense_call(x, op["kernel"], op["bias"], 4)
        p = ((v * inv).astype(F32) + shift).astype(F32)
        _DENSE[dc["id"]] = (x, op, inv, shift, p)
    return _DENSE[dc["id"]]
