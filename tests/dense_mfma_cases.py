"""Dense layers for the register-fed GEMM k_dense_mfma (csrc/qnn_dense_mfma.hip): a restatement of its host plan and of its
route rule, and four groups of cases with bit-exact references.  A plain module (no tests in it): test_dense_plan.py holds
plan() to the C++ header, test_dense_mfma_cases_cpu.py proves what the table covers and carries, and
test_gpu_wide_dense_mfma_grid.py runs every case on the kernel and on its VALU twin.

References: the contraction is an exact integer product of the codes (float64 matrix product of integers, every sum
asserted below 2^53), scaled by the power-of-two code scales and rounded once to float32 (for the small layers also held
to tail_cases.dense_contraction, int64, by the CPU test); the float32 chain behind it is tail_cases.dense_epilogue (the
oracle's bias_add and batchnorm_inference, in the ABI's order) and the activations of epilogue_grid_cases.ACT.

Group A  the epilogue on exact points (the recipe of epilogue_grid_cases.base on a dense layer): every pre-activation a
         small dyadic number, with rounding ties, exact zeros and clip edges among them.
Group B  every tile width and every K split the plan can choose, on every (operand store, output store) pair.
Group C  saturated operands up to the route's cin limit, where the int32 accumulator passes 2^24 and reaches 2^30.
Group D  activations narrower than their store against binary, ternary and narrow quantized weights.

What differs from a first reading of the shapes one would pick for group A, and why:
  * N.  A special point is ONE accumulator value per unit, and the accumulator of K = 192 products has a standard deviation
    of 40 (4-bit recipe), 23 (8-bit recipe) or 14 (+-1), so no value is taken by more than 1 %, 1.7 % or 5.7 % of the
    outputs.  33 images x 48 units = 1584 outputs cannot hold 32 exact zeros on 4- or 8-bit operands whatever the bias and
    BN tables are.  The floors stay; the layers have 527 images (packed outputs) and 79 (float32 outputs; the route takes
    BIN -> float32 above 64 images only): 32 whole image tiles (4) and a ragged tile of 15 rows.  The
    plan is still NT = 1, ks = 4 (one round of workgroups).
  * bias.  bias = align + delta: delta is the recipe's table (multiples of 2^-4; BIN: even integers); align = mean - beta /
    inv of the variant's BN (a multiple of 2^-4, 0 without BN) centres the BN on the accumulator's narrow range, as the 8-bit
    sums (|v| < 0.5) would otherwise meet zero only in the few units whose BN constants cancel by themselves.
  * BIN.  +-1 sums plus an even bias are even integers: without BN they clip everywhere and carry exact zeros only; behind
    a BN their ties need inv <= 1/16 (Q(2)) and 1/32 (Q(4)), so the BIN layers scale dyadic_bn's gamma by 1/16.
  * the "nobias" variant carries a BN with mean 0 (nothing to align it with).
claims() says which points a (case, activation) must carry; where it says no, the CPU test states why no input reaches them.
The "faithful" trick constants are NOT in the table: the reference's Dense layers have no such chain (binary_layers.py:78-85;
oracle binary_dense_call) and qnn_dense_forward refuses trick_s != 0 before any route is asked."""
import zlib

import numpy as np

from oracle import qnn_oracle as O
import epilogue_grid_cases as G
import qact_grid_cases as QG
import tail_cases as T

F32 = np.float32
SF32, BIN, I4, I8 = T.STORE_F32, T.STORE_BIN, T.STORE_I4, T.STORE_I8
NAME = T.STORE_NAME
QT, BT, RELU, LEAKY = "quantized_tanh", "binary_tanh", "quantized_relu", "quantized_leakyrelu"
PAIRS = ((I4, I4), (I4, I8), (I4, SF32), (I8, I4), (I8, I8), (I8, SF32), (BIN, I4), (BIN, SF32))     # (XS, OUT) of the route
_PAIR = {BIN: (1, "binary", 1), I4: (4, "quantized", 4), I8: (8, "quantized", 8)}                    # full-width operands
CUS = 256
RESIDENT, FILL, MEET = 4, 8, 2                      # kDenseResident, kDenseFill, kDenseMeet (csrc/qnn_dense_plan.h)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ---------------------------------------------------------------------------------------------------------------------
# the host plan and the K shares (csrc/qnn_dense_plan.h, k_dense_mfma)
# ---------------------------------------------------------------------------------------------------------------------
def plans(N, units, steps, cus=CUS):
    """dense_plan restated on int64 arrays of equal shape: (ok, nt, ks, ublocks, blocks); ok False where it refuses."""
    N, units, steps = (np.asarray(a, dtype=np.int64) for a in (N, units, steps))
    ok = (N >= 1) & (units >= 16) & (steps >= 1) & (cus >= 1)
    itiles, utiles, cap = -(-N // 16), -(-units // 16), max(cus, 1) * RESIDENT
    best = np.full(N.shape, np.iinfo(np.int64).max)
    got = [np.zeros(N.shape, np.int64) for _ in range(4)]
    for nt in (4, 2, 1):
        for ks in (1, 2, 4):
            ub, per = -(-utiles // nt), 4 // ks
            blocks = ub * -(-itiles // per)
            walk = -(-steps // ks) * (nt + 1) + FILL + (MEET if ks > 1 else 0)
            cost = -(-blocks // cap) * walk
            take = (cost < best) & (blocks < 2 ** 31)            # the first of the lowest cost wins
            best = np.where(take, cost, best)
            for g, v in zip(got, (nt, ks, ub, blocks)):
                g[take] = v[take] if isinstance(v, np.ndarray) else v
    return (ok & (best < np.iinfo(np.int64).max),) + tuple(got)


def plan(N, units, steps, cus=CUS):
    """One call: (nt, ks, ublocks, blocks), or None where dense_plan refuses."""
    ok, *got = plans([N], [units], [steps], cus)
    return tuple(int(g[0]) for g in got) if ok[0] else None


def shares(steps, ks):
    """K-steps each of the ks waves along K walks: share = ceil(steps / ks), wave kp takes [kp * share, min(kp * share + share,
    steps)) -- the last share may be short, the later ones empty."""
    share = -(-steps // ks)
    return [max(0, min(kp * share + share, steps) - kp * share) for kp in range(ks)]


def case_plan(c):
    return plan(c["N"], c["units"], c["K"] // 64)


def route(c):
    """Does qnn_route_dense_mfma take the call?  Its predicates, in its order (none of these cases has a shortcut, the
    trick or a scaled input, which the route list keeps from it)."""
    xs, out, K, U, N = c["x_store"], c["out_store"], c["K"], c["units"], c["N"]
    if c.get("w_store", xs) != xs or xs not in (I4, I8, BIN):
        return False
    if K % 64 != 0 or K > 65536 or U % 16 != 0:
        return False
    if out != SF32 and out != I4 and not (out == I8 and xs != BIN):
        return False
    if out == SF32 and U <= 256:
        return False
    if xs == BIN and out == SF32 and N <= 64:
        return False
    if any(fn not in ("none", BT, QT, RELU, LEAKY) for fn, _ in c["acts"]):
        return False
    if N * U >= 2 ** 31 or N * T.words(xs, K) >= 2 ** 31:
        return False
    return case_plan(c) is not None


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def weight_codes(c, d):
    wq, wshift = T.quantized_kernel(c, d["kernel"])
    codes = np.rint(wq.astype(np.float64) * 2.0 ** wshift)
    assert np.array_equal(codes * 2.0 ** -wshift, wq.astype(np.float64))
    return codes, wshift


def accumulator(c, d):
    """The exact integer sums (N, units), int64: a float64 matrix product of integer codes whose every partial sum stays
    below 2^53 in any order."""
    wcodes, _ = weight_codes(c, d)
    x = d["codes"].astype(np.float64)
    assert c["K"] * np.abs(x).max() * np.abs(wcodes).max() < 2.0 ** 53
    acc = x @ wcodes
    assert np.array_equal(acc, np.rint(acc))
    return acc.astype(np.int64)


def contraction(c, d, acc=None):
    """float32(acc * 2^-(xshift + wshift)): the integer sum, scaled exactly, rounded once."""
    acc = accumulator(c, d) if acc is None else acc
    _, wshift = weight_codes(c, d)
    return (acc.astype(np.float64) * (T.code_scale(c["x_store"], c["x_bits"]) * 2.0 ** -wshift)).astype(F32)


def activation(fn, nb, p):
    return p if fn == "none" else G.ACT[fn](p, nb)


_LAYERS = {}


def layer(c):
    """(inputs d, accumulator -- group C only --, pre-activation) of a case: built once per c["layer"] and shared by the case's activations and
    by the cases (output stores) that name the same layer.  Nothing in it is ever written again."""
    key = c["layer"]
    if key not in _LAYERS:
        d = c["inputs"](c)
        acc = accumulator(c, d)
        pre = T.dense_epilogue(dict(c, fn="none"), d, contraction(c, d, acc))
        for a in (d["codes"], d["kernel"], acc, pre):
            a.setflags(write=False)
        _LAYERS[key] = (d, acc if c["group"] == "C" else None, pre)       # (the sums are kept where a test reads them)
    return _LAYERS[key]


def reference(c, fn, nb):
    """Expected float32 output (N, units) of activation (fn, nb) of case c; a packed output holds the codes of these."""
    return activation(fn, nb, layer(c)[2])


def codes_of(fn, nb, values):
    """Integer codes of a packed output (tail_cases.out_codes)."""
    return T.out_codes(dict(out_store=I4, fn=fn, act_bits=nb), values)


def _case(group, xs, xb, wkind, wb, N, K, U, out, acts, inputs, layer_key, tag, **kw):
    c = T._case(xs, xb, wkind, wb, N, K, U, out_store=out, **kw)
    c.update(group=group, acts=list(acts), inputs=inputs, layer=(group, xs, xb, wkind, wb, N, K, U) + tuple(layer_key),
             id="%s-%s%d-%s%d-o%s-N%d-K%d-U%d%s" % (group, NAME[xs], xb, wkind[0], wb, NAME[out], N, K, U, "-" + tag if tag else ""))
    c["seed"] = _seed(*c["layer"]) % (2 ** 31)
    c["on_route"] = True                                    # what the case claims; the CPU test holds route(c) to it
    return c


# ---------------------------------------------------------------------------------------------------------------------
# group A: the epilogue on exact points
# ---------------------------------------------------------------------------------------------------------------------
A_N = {"packed": 527, "f32": 79, "bin_f32": 79}
A_K = 192
A_VARIANTS = ("pos", "neg", "mixed", "nobn", "nobias")
# The 8-bit sums are tiny (|v| < 0.5, a step of 1/256), so a unit of an 8-bit layer meets a point only where its constants
# put it there.  TARGET8 lists, in units of 2^-4, the pre-activation a unit has at s = 0, by unit mod 19 (19: every target
# visits every position of a 16-unit tile): 0 (zeros, the lower edge region of quantized_relu with -1, -2 and 1), +-4 and
# -12 (ties of Q(2)), the odd values (ties of Q(4), quantized_relu and quantized_leakyrelu at 4 bits), -16 / 16 / 14 / 8
# (clip edges of every width; Q(8)'s upper edge 127/128 lies at s = -2 beside 16), 14 and 15 (upper edge region of the
# ReLU forms), -10 (the negative tie -5/8 of leaky Q(4)).  The bias delta of unit u is TARGET8 / (16 inv_u): a multiple of
# 2^-4, as 1 / |inv| is 1, 2, 4 or 8; the "nobias" variant carries the targets as its beta.
# (the targets that only an edge claims stand at 6 .. 8 and 16 .. 18, so that each tile position of a 48-unit layer, which
# sees the entries p, p - 3 and p + 13, has at least one tie or zero target)
TARGET8 = (0, 4, 1, -4, 3, -12, -16, 16, 14, 0, -1, 5, -10, 0, -3, 7, 15, 8, -2)
ACTS_A = {I4: ((QT, 2), (QT, 4), (BT, 0), (RELU, 4), (LEAKY, 4)),
          I8: ((QT, 8), (QT, 4), (RELU, 8)),
          SF32: (("none", 0), (BT, 0), (QT, 4), (QT, 8), (LEAKY, 4))}


def a_bn(xs, U, variant):
    """The BN dict of a group A variant (None for "nobn"), see the module docstring."""
    if variant == "nobn":
        return None
    bn = dict(G.dyadic_bn(U, "mixed" if variant == "nobias" else variant))
    if variant == "nobias":
        bn["mean"] = np.zeros(U, F32)
    if xs == BIN:
        bn["gamma"] = (bn["gamma"] / F32(16)).astype(F32)
    return bn


def _a_inputs(c):
    xs, N, K, U, variant = c["x_store"], c["N"], c["K"], c["units"], c["variant"]
    rng = np.random.default_rng(_seed("A", xs, N, K, U))                   # the same tensors under every variant
    u = np.arange(U)
    if xs == BIN:
        codes = rng.integers(0, 2, (N, K)) * 2 - 1
        kernel = ((rng.integers(0, 2, (K, U)) * 2 - 1) * 0.5).astype(F32)
        delta = rng.integers(-1, 2, U) * 2.0
    elif xs == I4:
        codes = np.clip(np.rint(rng.standard_normal((N, K)) * 2), -8, 7)
        kernel = (rng.integers(-2, 3, (K, U)) / 8.0).astype(F32)
        delta = rng.integers(-4, 5, U) / 16.0
    else:
        codes = np.clip(np.rint(rng.standard_normal((N, K)) * 2) * 8, -128, 127)
        kernel = (rng.integers(-1, 2, (K, U)) * 8 / 128.0).astype(F32)
        delta = np.array(TARGET8)[u % len(TARGET8)] / 16.0
    bn = a_bn(xs, U, variant)
    if xs == I8 and bn is not None:
        if variant == "nobias":
            bn["beta"] = delta.astype(F32)
        else:
            inv, _ = O.bn_constants(bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"])
            delta = delta / inv.astype(np.float64)
    bias = None
    if variant != "nobias":
        align = np.zeros(U)
        if bn is not None:
            inv, shift = O.bn_constants(bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"])
            align = -shift.astype(np.float64) / inv.astype(np.float64)
            assert np.array_equal(align * 16, np.rint(align * 16))
        bias = (align + delta).astype(F32)
        assert np.array_equal(bias.astype(np.float64), align + delta) and np.array_equal(bias * 16, np.rint(bias * 16))
    codes = codes.astype(np.int8)
    x = (codes.astype(np.float64) * T.code_scale(xs, c["x_bits"])).astype(F32)
    return dict(codes=codes, x=x, kernel=kernel, bias=bias, bn=bn, res=None, post_scale=1.0)


def claims(c, fn, nb):
    """What the CPU test demands of activation (fn, nb) of a group A case: a set out of "ties", "zeros", "edges", "neg".
    Points that no input of the case's operand recipe reaches are not claimed (the CPU test asserts that they do not occur):
      * BIN without BN: even integers, every quantized activation is clipped; exact zeros only.
      * 4-bit operands without BN: v * 128 = 2 acc + 8 (16 bias) is an integer, Q(8) has no tie.
      * clip edges are claimed where the grid reaches them by itself, i.e. without BN (as test_epilogue_grid_cpu.py does);
        BIN never reaches one (the lower edge -1 is odd, the upper edges are no integers).
      * BIN behind its BN: inv >= 1/128, so p * 128 is an integer and Q(8) has no tie."""
    xs, nobn = c["x_store"], c["variant"] == "nobn"
    if fn == "none":
        return set()
    if fn == BT:
        return {"zeros"}
    if xs == BIN and nobn:
        return set()
    if (xs == I4 and nobn and nb == 8) or (xs == BIN and nb == 8):       # (BIN: p * 128 = (s + delta) * 128 inv, an integer)
        return set()
    out = {"ties"}
    if nobn and xs != BIN:
        out.add("edges")
    if fn == LEAKY:
        out.add("neg")
    return out


def special(p, fn, nb):
    """Mask of the points of p that decide (fn, nb): exact zeros for binary_tanh, the ties of the quantized activations."""
    p64 = p.astype(np.float64)
    if fn == BT:
        return p == 0
    m = 2.0 ** (nb - 1)
    if fn == QT:
        t = p64 * m
        return (t - np.floor(t) == 0.5) & (t > -m) & (t < m - 1)
    t, off, lo = QG._t(p, fn, nb)
    return QG._frac_half(t) & (t - off > lo) & (t - off < m - 1)


def _group_a():
    t = []
    for xs in (I4, I8, BIN):
        xb, wk, wb = _PAIR[xs]
        for variant in A_VARIANTS:
            for out in (o for x, o in PAIRS if x == xs):
                N = A_N["packed"] if out != SF32 else A_N["bin_f32"] if xs == BIN else A_N["f32"]
                U = 48 if out != SF32 else 272
                c = _case("A", xs, xb, wk, wb, N, A_K, U, out, ACTS_A[out], _a_inputs, (variant,), variant, bias=variant != "nobias",
                          bn=None if variant == "nobn" else variant)
                c["variant"] = variant
                t.append(c)
    return t


# ---------------------------------------------------------------------------------------------------------------------
# groups B, C, D: the inputs of tail_cases.dense_inputs
# ---------------------------------------------------------------------------------------------------------------------
def _t_inputs(c):
    """tail_cases.dense_inputs with both signs of gamma (odd units negative), and for "dent" cases the first activation code
    of image n lowered by 1 + n, so that saturated sums differ per image and stop being multiples of a high power of two."""
    d = T.dense_inputs(c)
    if d["bn"] is not None:
        d["bn"]["gamma"][1::2] *= F32(-1)
    if c.get("dent"):
        codes = d["codes"].copy()
        codes[:, 0] -= (1 + np.arange(c["N"])).astype(np.int8)
        assert codes[:, 0].min() >= T.code_range(c["x_store"], c["x_bits"])[0]
        d["codes"] = codes
        d["x"] = (codes.astype(np.float64) * T.code_scale(c["x_store"], c["x_bits"])).astype(F32)
    return d


B_TILES = ((2049, 64, 528, (2, 1)), (513, 192, 528, (2, 4)), (1025, 384, 528, (2, 2)), (2049, 64, 1040, (4, 1)),
           (2049, 256, 528, (4, 2)), (1025, 256, 528, (4, 4)))
B_12 = (16401, 256, 16, (1, 2))
B_SHARES = ((17, 128, 32, [2]), (17, 320, 32, [2, 2, 1, 0]), (17, 448, 48, [2, 2, 2, 1]), (17, 576, 48, [3, 3, 3, 0]),
            (33, 1088, 32, [5, 5, 5, 2]))
B_ACT = {(I4, I4): (QT, 4), (I4, I8): (QT, 8), (I4, SF32): ("none", 0), (I8, I4): (QT, 4), (I8, I8): (QT, 8),
         (I8, SF32): (QT, 8), (BIN, I4): (BT, 0), (BIN, SF32): ("none", 0)}


def _b_case(xs, out, N, K, U, want, tag):
    xb, wk, wb = _PAIR[xs]
    assert K * 4 ** (xb - 1) <= 2 ** 24                      # (every sum is also a float32, as in test_gpu_wide_dense_mfma.py)
    c = _case("B", xs, xb, wk, wb, N, K, U, out, [B_ACT[xs, out]], _t_inputs, (), tag, bn="pos")
    c["want_plan"] = want
    return c


def _group_b():
    t = []
    for N, K, U, want in B_TILES:
        t += [_b_case(xs, out, N, K, U, want, "nt%dks%d" % want) for xs, out in PAIRS]
    N, K, U, want = B_12
    t += [_b_case(xs, xs, N, K, U, want, "nt1ks2") for xs in (I4, I8)]
    for N, K, U, sh in B_SHARES:
        for xs in (I4, BIN):
            c = _b_case(xs, I4, N, K, U, (1, len(sh)), "shares" + "".join(map(str, sh)))
            c["want_shares"] = sh
            t.append(c)
    return t


C_FILLS = ("max", "min", "alternating", "min_max")
C_ACT = {I8: (QT, 8), I4: (QT, 4), BIN: (BT, 0)}


def _c_case(xs, N, K, U, fill, dent=False, bn="pos", bias=True):
    xb, wk, wb = _PAIR[xs]
    out = SF32 if U > 256 else I4 if xs == BIN else xs
    c = _case("C", xs, xb, wk, wb, N, K, U, out, [("none", 0) if out == SF32 else C_ACT[xs]], _t_inputs, (fill, dent, bn, bias),
              fill + ("-dent" if dent else "") + ("" if bn else "-nobn"), fill=fill, bn=bn, bias=bias)
    c["dent"] = dent
    return c


def _group_c():
    t = []
    for fill in C_FILLS:
        for xs in (I8, I4, BIN):
            t.append(_c_case(xs, 5, 4608, 16, fill))
            if xs != BIN:                                   # (BIN -> float32 stays off the route at 5 images)
                t.append(_c_case(xs, 5, 4608, 272, fill))
    # the fills' own sums are multiples of 2^8 and more, exact in float32 even above 2^24 (127 * 127 * 4608 = 145161 * 2^9):
    # the dented rows are the ones whose int32 -> float32 conversion rounds (once onto a tie: image 3, -508 = 4 mod 8)
    t.append(_c_case(I8, 5, 4608, 16, "max", dent=True))
    t.append(_c_case(I8, 5, 4608, 272, "max", dent=True, bn=None, bias=False))
    t.append(_c_case(I8, 5, 65536, 16, "max", dent=True))
    for K in (65536, 65600):                                # the cin limit of the route, and the first K % 64 == 0 past it
        for fill in ("min", "min_max"):
            for xs in (I8, I4):
                t.append(_c_case(xs, 5, K, 16, fill))
                t[-1]["on_route"] = K <= 65536
    return t


def _group_d():
    t = []
    rows = [(I4, xb, wk, wb) for xb in (1, 2, 3) for wk, wb in (("binary", 1), ("ternary", 1), ("quantized", 2))] + \
           [(I8, xb, wk, wb) for xb in (3, 5) for wk, wb in (("binary", 1), ("ternary", 1), ("quantized", 5))]
    for xs, xb, wk, wb in rows:
        t.append(_case("D", xs, xb, wk, wb, 17, 192, 48, I4, [(QT, 4)], _t_inputs, (), "", bn="pos"))
        t.append(_case("D", xs, xb, wk, wb, 17, 192, 272, SF32, [("none", 0)], _t_inputs, (), "", bn="pos"))
    return t


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        t = _group_a() + _group_b() + _group_c() + _group_d()
        assert len({c["id"] for c in t}) == len(t)
        _CASES = t
    return _CASES


def group(g):
    return [c for c in cases() if c["group"] == g]
