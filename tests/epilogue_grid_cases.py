"""Convolution layers whose pre-activations land exactly on the points where an epilogue can go wrong: the rounding ties of
quantized_tanh (v * 2^(nb-1) a half-integer; the reference rounds half to even), the threshold of binary_tanh (+1 iff
v > 2^-24, so an exact 0 maps to -1) and the clip edges (v * m equal to -m or m - 1).  A plain module (no tests in it): the
CPU test (test_epilogue_grid_cpu.py) proves that every case carries enough of these points and that they tell a wrong
rounding or threshold from the right one; the GPU test (test_gpu_epilogue_grid.py) runs each case on the kernel it names.

Everything is on a grid: activation codes with a small spread, weight codes in -2 .. 2, biases that are multiples of 2^-4,
BatchNorm constants whose scale is a power of two and whose shift is a multiple of 2^-4, shortcut codes (or float32
shortcut values that are multiples of 2^-4).  Every intermediate value is then a small dyadic number, exact in float32
in any evaluation order: the kernels have no rounding to hide behind.

The expected output comes from oracle/qnn_oracle.py alone (the conv call with its bias_add, batchnorm_inference, the add
and scale of the residual merge, quantized_tanh / binary_tanh, maxpool2d)."""
import zlib

import numpy as np

from oracle import qnn_oracle as O
import conv_dilation_cases as D
import qrelu_cases as Q

F32 = np.float32
STORE_F32, STORE_BIN, STORE_I4, STORE_I8 = 0, 1, 4, 8                        # include/qnn_abi.h
EPI_NO_STRIP, EPI_NO_STRIP64, EPI_NO_HALO = 1, 2, 4                         # qnn_epilogue_t.flags
STORE_NAME = {STORE_F32: "f32", STORE_BIN: "bin", STORE_I4: "i4", STORE_I8: "i8"}
MIN_TIES, MIN_ZEROS, MIN_EDGE, MIN_DIFF = 32, 32, 8, 8
# Values of the residual merge planted through the shortcut (see shortcut()), per activation of the case: exact zeros for
# binary outputs, the ties nearest to zero for Q(2), Q(4) and Q(8); (target, positions).  A third element "f32" marks a
# target that is no dyadic number (the float32 neighbour of one): only a float32 shortcut can carry it, on positions where
# r = T / post_scale - v is a float32 and r + v is exact.  A case may carry a table of its own as c["plant"] (qact_grid_cases.py: its two functions).
PLANT = {("binary_tanh", 0): ((0.0, 64),), ("quantized_tanh", 2): ((0.25, 32), (-0.25, 32), (-0.75, 32)),
         ("quantized_tanh", 4): ((1 / 16, 32), (-1 / 16, 32), (3 / 16, 32), (-3 / 16, 32)),
         ("quantized_tanh", 8): ((1 / 256, 32), (-1 / 256, 32), (3 / 256, 32), (-3 / 256, 32))}


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ---------------------------------------------------------------------------------------------------------------------
# tensors
# ---------------------------------------------------------------------------------------------------------------------
_BASES = {}
# bias of the 8-bit layers in units of 2^-4, by channel mod 16: mostly near zero (exact zeros for the binary outputs), two
# channels at -1 and +1 (the clip edges of Q(8), the lower one of Q(4)) and one at 14 / 16 (the upper clip edge of Q(4))
BIAS8 = (0, 0, 1, -1, 0, 2, -2, 0, -16, 16, 0, 1, -1, 0, 0, 14)


def base(x_store, N, H, W, cin, cout, k=3, stride=1, bias=True, d=1):
    """Inputs, layer and plain convolution (bias included) of one (input store, geometry): built once and shared.
    d: a square dilation rate; the op carries it as dilation_rate, the oracle convolves with the zero-stuffed kernel
    (conv_dilation_cases.stuff, proven by test_conv_dilation_cpu.py).

    4-bit operands: activation codes rint(normal * 2) (values of about 0.25 sigma), weight codes -2 .. 2, so the conv value is
    acc / 64.  8-bit operands: activation codes 8 * rint(normal * 2), weight codes 8 * (-1 .. 1): the conv value is S / 256,
    which puts Q(8) ties at odd S and Q(4) ties at S = 16 mod 32; such small sums reach the clip edges of Q(8) only through
    the bias, hence BIAS8.  BIN: +-1 against +-1.  The bias is a multiple of 2^-4 (BIN: an even integer, as the sum of an
    even number of +-1 is even)."""
    key = (x_store, N, H, W, cin, cout, k, stride, bias) + ((d,) if d != 1 else ())
    if key in _BASES:
        return _BASES[key]
    rng = np.random.default_rng(_seed("base", *key))
    if x_store == STORE_BIN:
        xb = 1
        x = (rng.integers(0, 2, (N, H, W, cin)) * 2 - 1).astype(F32)
        kernel = ((rng.integers(0, 2, (k, k, cin, cout)) * 2 - 1) * 0.5).astype(F32)
        op = {"op": "conv", "kind": "binary", "kernel": kernel}
        b = (rng.integers(-1, 2, cout) * 2).astype(F32)
        wq = O.binarize(kernel)
    else:
        xb = x_store or 4                            # (a float32 input carries values of the 4-bit grid)
        m = 2.0 ** (xb - 1)
        if xb == 4:
            a = np.rint(rng.standard_normal((N, H, W, cin)) * 2)
            wc = rng.integers(-2, 3, (k, k, cin, cout))
            b = (rng.integers(-4, 5, cout) / 16.0).astype(F32)
        else:
            a = np.rint(rng.standard_normal((N, H, W, cin)) * 2) * 8
            wc = rng.integers(-1, 2, (k, k, cin, cout)) * 8
            b = (np.array(BIAS8)[np.arange(cout) % 16] / 16.0).astype(F32)
        x = (np.clip(a, -m, m - 1) / m).astype(F32)
        kernel = (wc / m).astype(F32)
        op = {"op": "conv", "kind": "quantized", "nb": xb, "kernel": kernel}
        wq = O.quantize(kernel, xb)
        assert np.array_equal(O.quantized_tanh(x, xb), x)
    assert np.array_equal(wq, kernel if x_store != STORE_BIN else np.sign(kernel))        # the latent kernel is on the grid
    op.update(bias=b if bias else None, strides=(stride, stride), padding="same")
    if d != 1:
        assert x_store != STORE_BIN                   # (a stuffed kernel never goes through binarize)
        op["dilation_rate"] = (d, d)
    if x_store == STORE_BIN:
        conv = O.binary_conv2d_call(x, kernel, op["bias"], strides=op["strides"])
    else:
        conv = O.quantized_conv2d_call(x, D.stuff(kernel, d, d), op["bias"], nb=xb, strides=op["strides"])
    _BASES[key] = dict(key=key, x=x, x_bits=xb, op=op, conv=conv)
    return _BASES[key]


_BNS = {}


def dyadic_bn(cout, sign):
    """BN parameters from which bn_constants (tf.nn.batch_normalization's inv = rsqrt(var + eps) * gamma, shift = beta -
    mean * inv) forms a power-of-two inv in {1/8, 1/4, 1/2, 1} and a shift that is a multiple of 2^-4, exactly: var + eps is
    1 or 4.  sign: "pos", "neg" (every scale negative) or "mixed" (channels 1 mod 3 negative: both signs inside every 16-,
    32- and 64-filter slice).  "wide": the mixed pattern with four times the scale, {1/2, 1, 2, 4}: pre-residual values of
    several units, for a shortcut merge scaled by 1/4 that must still reach a point away from zero."""
    if (cout, sign) not in _BNS:
        c = np.arange(cout)
        s = {"pos": np.ones(cout), "neg": -np.ones(cout), "mixed": np.where(c % 3 == 1, -1.0, 1.0),
             "wide": np.where(c % 3 == 1, -4.0, 4.0)}[sign]
        bn = dict(op="bn", eps=0.25, gamma=(s * np.array([0.25, 0.5, 1.0, 0.25])[c % 4]).astype(F32),
                  var=np.array([0.75, 3.75])[(c // 4) % 2].astype(F32), mean=(((c % 3) - 1) * 0.5).astype(F32),
                  beta=(((c % 5) - 2) / 16.0).astype(F32))
        inv, shift = O.bn_constants(bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"])
        assert np.all(np.abs(np.frexp(inv)[0]) == 0.5) and np.all(np.abs(inv) >= (0.5 if sign == "wide" else 0.125)) and \
            np.all(np.abs(inv) <= (4 if sign == "wide" else 1))
        assert np.array_equal(shift * 16, np.rint(shift * 16)) and np.array_equal(np.sign(inv), np.sign(s))
        _BNS[cout, sign] = bn
    return _BNS[cout, sign]


def pre_residual(c):
    """The oracle's value in front of the residual merge: conv + bias [-> BN]."""
    v = base(*c["base"])["conv"]
    if c["sign"] is not None:
        bn = dyadic_bn(c["base"][5], c["sign"])
        v = O.batchnorm_inference(v, bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"])
    return v


_SHORTCUTS = {}


def shortcut(c):
    """float32 values of the case's shortcut (None without one): codes rint(normal * 0.25 * 2^(res_bits-1)) of res_bits, or
    float32 multiples of 2^-4.  Then the special points of the case's activations are planted: for every (target T, count)
    of PLANT, on positions spread over the tensor where r = T / post_scale - v (v = pre_residual) is itself a shortcut
    value, the shortcut is that r, so that the merge (r + v) * post_scale is exactly T.  A target takes at most a third
    of the positions still open to it, so that the later ones find some too.  An "f32" target (see PLANT) is skipped by
    a packed shortcut; a float32 one takes the positions where r is a float32 and the float32 sum r + v is T / post_scale."""
    if c["res"] is None:
        return None
    table = c.get("plant") or PLANT
    targets = tuple(t for k in sorted({(a["fn"], a["nb"]) for a in c["acts"]}) for t in table[k])
    key = (c["base"], c["sign"], c["res"], c["res_bits"], c["post_scale"], targets)
    if key not in _SHORTCUTS:
        v = pre_residual(c).astype(np.float64)
        rng = np.random.default_rng(_seed("shortcut", *key))
        if c["res"] == STORE_F32:
            m, lo, hi = 2.0 ** 20, -4.0, 4.0
            r = np.rint(rng.standard_normal(v.shape) * 4) / 16.0
        else:
            m = 2.0 ** (c["res_bits"] - 1)
            lo, hi = -1.0, (m - 1) / m
            r = np.clip(np.rint(rng.standard_normal(v.shape) * 0.25 * m), -m, m - 1) / m
        free = np.ones(v.size, bool)
        for T, count, *exact in targets:
            want = (T / c["post_scale"] - v).reshape(-1)
            if exact:
                if c["res"] != STORE_F32:
                    continue
                w32 = want.astype(F32)
                ok = (w32.astype(np.float64) == want) & ((w32 + v.reshape(-1).astype(F32)).astype(np.float64) == T / c["post_scale"])
            else:
                ok = want * m == np.rint(want * m)
            idx = np.flatnonzero(ok & (want >= lo) & (want <= hi) & free)
            n = min(count, (idx.size + 2) // 3)
            idx = idx[np.unique(np.linspace(0, idx.size - 1, n).astype(np.int64))] if n else idx[:0]
            r.reshape(-1)[idx] = want[idx]
            free[idx] = False
        _SHORTCUTS[key] = r.astype(F32)
        assert np.array_equal(_SHORTCUTS[key].astype(np.float64), r)
    return _SHORTCUTS[key]


def preactivation(c):
    """The oracle's float32 value the activation is applied to (before pooling)."""
    v = pre_residual(c)
    r = shortcut(c)
    if r is not None:
        v = ((r + v).astype(F32) * F32(c["post_scale"])).astype(F32)        # keras.layers.add, Lambda(x * post_scale)
    return v


def _pool(c, y):
    return O.maxpool2d(y) if c["pool"] == 2 else y


# the activations by name: the oracle's two, and the restatements of qrelu_cases.py (held to golden/ref_qrelu.npz)
ACT = {"binary_tanh": lambda p, nb: O.binary_tanh(p), "quantized_tanh": O.quantized_tanh,
       "quantized_relu": Q.quantized_relu, "quantized_leakyrelu": Q.quantized_leakyrelu}


def expected(c, a, p=None):
    """The oracle's output of activation `a` of case `c`: float32 values (a packed output holds their codes)."""
    p = preactivation(c) if p is None else p
    return _pool(c, ACT[a["fn"]](p, a["nb"]))


# ---------------------------------------------------------------------------------------------------------------------
# what a case must carry, counted on the pre-activation
# ---------------------------------------------------------------------------------------------------------------------
def tie_count(p, nb):
    """Pre-activations whose p * m is a half-integer with both neighbours inside the clip range [-m, m - 1]."""
    m = 2.0 ** (nb - 1)
    t = p.astype(np.float64) * m
    return int(np.count_nonzero((t - np.floor(t) == 0.5) & (t > -m) & (t < m - 1)))


def zero_count(p):
    return int(np.count_nonzero(p == 0))


def edge_counts(p, nb):
    m = 2.0 ** (nb - 1)
    t = p.astype(np.float64) * m
    return int(np.count_nonzero(t == -m)), int(np.count_nonzero(t == m - 1))


def _requantize(c, t, nb):
    m = 2.0 ** (nb - 1)
    return _pool(c, (np.clip(t, -m, m - 1) / m).astype(F32))


def wrong_half_away(c, p, nb):
    """quantized_tanh with ties rounded away from zero."""
    t = p.astype(np.float64) * 2.0 ** (nb - 1)
    return _requantize(c, np.sign(t) * np.floor(np.abs(t) + 0.5), nb)


def wrong_floor_half(c, p, nb):
    """quantized_tanh as floor(x + 0.5): ties rounded up."""
    t = p.astype(np.float64) * 2.0 ** (nb - 1)
    return _requantize(c, np.floor(t + 0.5), nb)


def wrong_binary_ge0(c, p):
    """binary_tanh with `>= 0` as its threshold."""
    return _pool(c, np.where(p >= 0, F32(1), F32(-1)).astype(F32))


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
def A(fn, nb, store, named=True):
    """One activation / output store of a case.  named: the call must run on the case's kernel (False: the store selects
    another kernel; the output is compared all the same)."""
    return dict(fn=fn, nb=nb, store=store, named=named,
                id="%s%s" % ({"binary_tanh": "b", "quantized_tanh": "q%d", "quantized_relu": "relu%d",
                              "quantized_leakyrelu": "leaky%d"}[fn].replace("%d", str(nb)), STORE_NAME[store]))


QT, BT = "quantized_tanh", "binary_tanh"
# the int4 kernels that store packed int4 codes only (strip, small, halo); other stores of the same layer, unnamed
ACTS_I4 = [A(QT, 4, STORE_I4), A(QT, 2, STORE_I4), A(BT, 0, STORE_I4)]
ACTS_I4_MORE = ACTS_I4 + [A(QT, 4, STORE_F32, False), A(BT, 0, STORE_BIN, False), A(QT, 4, STORE_I8, False)]
# the kernels with every output store (areg, wres, tiles)
ACTS_ALL = ACTS_I4 + [A(QT, 4, STORE_I8), A(BT, 0, STORE_BIN), A(QT, 4, STORE_F32), A(QT, 2, STORE_F32), A(BT, 0, STORE_F32)]
ACTS_I8 = [A(QT, 8, STORE_I8), A(QT, 4, STORE_I8)]
ACTS_I8_ALL = ACTS_I8 + [A(BT, 0, STORE_I8), A(QT, 4, STORE_I4), A(BT, 0, STORE_BIN), A(QT, 8, STORE_F32), A(BT, 0, STORE_F32)]
ACTS_BIN = [A(BT, 0, STORE_BIN), A(BT, 0, STORE_F32, False)]


def _case(kernel, valu, x_store, shape, cout, acts, epi="nobn", sign=None, res=None, res_bits=0, post_scale=1.0, k=3,
          stride=1, pool=1, flags=0, bias=True, head=False, d=1):
    """kernel / valu: the names qnn_last_kernel reports in auto mode and under IMPL_VALU.  epi: "nobn", "dyadic" (sign:
    "pos" / "neg" / "mixed") or "residual" (res: STORE_I4 / STORE_I8 / STORE_F32, behind a dyadic BN when sign is set).
    d: a square dilation rate (see base)."""
    N, H, W, cin = shape
    assert (epi == "nobn") == (sign is None and res is None) and (epi == "residual") == (res is not None)
    c = dict(kernel=kernel, valu=valu, x_store=x_store,
             base=(x_store, N, H, W, cin, cout, k, stride, bias) + ((d,) if d != 1 else ()), acts=acts, d=d,
             epi=epi, sign=sign, res=res, res_bits=res_bits, post_scale=post_scale, pool=pool, flags=flags, head=head)
    tags = [kernel + ("+dense" if head else ""), "%dx%dx%dx%d" % shape + ("" if cout == cin else "-%d" % cout),
            "d%d" % d if d != 1 else None, "pool2" if pool == 2 else None, epi if epi != "dyadic" else sign, (sign or "nobn") if res is not None else None,
            None if res is None else "r%s%s" % (STORE_NAME[res], res_bits or ""), None if res is None else "x%g" % post_scale,
            None if bias else "nobias"]
    c["id"] = "-".join(t for t in tags if t)
    return c


def _ps(store, cin, k=3):
    return "ps_i%d_cw%d_k%d" % (store, cin * store // 32, k)


def _table():
    t = []
    I4, I8 = STORE_I4, STORE_I8
    # ---- the row-walking int4 strip kernels: 10 rows = chunks of 4, 4 and 2, 20 columns = a whole and a ragged strip
    for C in (16, 32, 64):
        name, valu, shape = "strip_i4_c%d" % C, _ps(4, C), (2, 10, 20, C)
        t.append(_case(name, valu, I4, shape, C, ACTS_I4_MORE))
        t.append(_case(name, valu, I4, shape, C, ACTS_I4, bias=False))
        t.append(_case(name, valu, I4, shape, C, ACTS_I4_MORE, "dyadic", "mixed"))
        t.append(_case(name, valu, I4, shape, C, ACTS_I4, "dyadic", "neg", bias=False))
        for post in (1.0, 0.5, 0.25):
            t.append(_case(name, valu, I4, shape, C, ACTS_I4, "residual", "mixed", I4, 4, post))
            t.append(_case(name, valu, I4, shape, C, ACTS_I4, "residual", None, I4, 2, post))
            t.append(_case(name, valu, I4, shape, C, ACTS_I4, "residual", "mixed" if post != 0.5 else None, STORE_F32, 0, post))
    for C in (16, 32):
        name, shape = "strip_i4_c%d_s2" % C, (2, 19, 21, C)
        t.append(_case(name, _ps(4, C), I4, shape, 2 * C, ACTS_I4_MORE, stride=2))
        t.append(_case(name, _ps(4, C), I4, shape, 2 * C, ACTS_I4, "dyadic", "mixed", stride=2))
    # ---- the dilated strip kernel (its own copy of the chain epilogue); under IMPL_VALU a dilated call runs on generic
    for C in (16, 32, 64):
        for d in (2, 3):
            name, shape = "strip_i4_c%d_dil" % C, (2, 10, 20, C)
            # (16 channels without BN: four images, as two hold 6 and 7 points on the lower clip edge of Q(2))
            t.append(_case(name, "generic", I4, (4, 10, 20, C) if C == 16 else shape, C, ACTS_I4, d=d))
            t.append(_case(name, "generic", I4, shape, C, ACTS_I4, "dyadic", "mixed", d=d))
            t.append(_case(name, "generic", I4, shape, C, ACTS_I4, "dyadic", "neg", bias=False, d=d))
            for post in (0.5, 1.0):
                t.append(_case(name, "generic", I4, shape, C, ACTS_I4, "residual", "mixed", I4, 4, post, d=d))
            t.append(_case(name, "generic", I4, shape, C, ACTS_I4, "residual", None, STORE_F32, 0, 0.5, d=d))
    # ---- the small-channel tile kernel
    for C in (16, 32):
        # (16 channels: four images, as two do not hold 32 exact zeros behind the dyadic BN)
        name, valu, shape = "mfma_i4_small_c%d" % C, _ps(4, C), (4 if C == 16 else 2, 9, 16, C)
        t.append(_case(name, valu, I4, shape, C, ACTS_I4, flags=EPI_NO_STRIP))
        t.append(_case(name, valu, I4, shape, C, ACTS_I4, "dyadic", "mixed", flags=EPI_NO_STRIP))
        t.append(_case(name, valu, I4, shape, C, ACTS_I4, "residual", "mixed", I4, 4, 0.5, flags=EPI_NO_STRIP))
        t.append(_case(name, valu, I4, shape, C, ACTS_I4, "residual", "mixed", STORE_F32, 0, 0.5, flags=EPI_NO_STRIP))
    # ---- 64 -> 64 channels: operands in registers (un-pooled with and without a shortcut, pooled), the halo kernel
    shape, valu = (2, 8, 16, 64), _ps(4, 64)
    t.append(_case("mfma_i4_areg64x64", valu, I4, shape, 64, ACTS_ALL, flags=EPI_NO_STRIP64))
    t.append(_case("mfma_i4_areg64x64", valu, I4, shape, 64, ACTS_ALL, "dyadic", "mixed", flags=EPI_NO_STRIP64))
    t.append(_case("mfma_i4_areg64x64", valu, I4, shape, 64, ACTS_ALL, "residual", "mixed", I4, 4, 0.5, flags=EPI_NO_STRIP64))
    for sign in (None, "pos", "neg", "mixed"):
        epi = "nobn" if sign is None else "dyadic"
        t.append(_case("mfma_i4_areg64x64", valu, I4, shape, 64, ACTS_ALL, epi, sign, pool=2, flags=EPI_NO_HALO))
        for shp in (shape, (3, 16, 16, 64)):
            t.append(_case("mfma_i4_halo64x64", valu, I4, shp, 64, ACTS_I4, epi, sign, pool=2))
    # ---- weight-resident 1x1 and the tiled kernels, N = 2 (whole 256-row tiles) and N = 3 (a ragged second tile)
    tiles = [("mfma_i4_wres256x64", I4, 64, 1), ("mfma_i4_256x64", I4, 192, 3), ("mfma_i4_256x128", I4, 128, 3),
             ("mfma_i4_256x256", I4, 256, 3), ("mfma_i8_256x128", I8, 128, 3), ("mfma_i8_256x256", I8, 256, 3)]
    for name, xs, cout, k in tiles:
        acts = ACTS_ALL if xs == I4 else ACTS_I8_ALL
        for N in (2, 3):
            for pool in (1, 2):
                kw = dict(k=k, pool=pool, flags=EPI_NO_STRIP64)
                t.append(_case(name, _ps(xs, 64, k), xs, (N, 8, 16, 64), cout, acts, **kw))
                t.append(_case(name, _ps(xs, 64, k), xs, (N, 8, 16, 64), cout, acts, "dyadic", "mixed", **kw))
                if pool == 2:
                    t.append(_case(name, _ps(xs, 64, k), xs, (N, 8, 16, 64), cout, acts, "dyadic", "neg", **kw))
    # ---- int8 operands: the pooled register kernel and the strip kernels
    for sign in (None, "pos", "neg", "mixed"):
        # (three images: behind the pool, two leave fewer than 8 outputs that an exact zero decides)
        t.append(_case("mfma_i8_areg64x64", _ps(8, 64), I8, (3, 8, 16, 64), 64, ACTS_I8_ALL, "nobn" if sign is None else "dyadic",
                       sign, pool=2))
    for C in (16, 32, 64):
        # (16 channels: three images, as one channel of two does not hold 8 points on the lower clip edge)
        name, valu, shape = "strip_i8_c%d" % C, _ps(8, C), (3 if C == 16 else 2, 10, 20, C)
        t.append(_case(name, valu, I8, shape, C, ACTS_I8))
        t.append(_case(name, valu, I8, shape, C, ACTS_I8, "dyadic", "mixed"))
        t.append(_case(name, valu, I8, shape, C, ACTS_I8, "residual", "mixed", I8, 8, 0.5))
        t.append(_case(name, valu, I8, shape, C, ACTS_I8, "residual", "mixed", I8, 4, 0.5))
        t.append(_case(name, valu, I8, shape, C, ACTS_I8, "residual", None, STORE_F32, 0, 0.5))
    # ---- BIN -> BIN on the XNOR kernel, and a channel count only k_conv_generic takes
    t.append(_case("xnor_pk_cw2", "xnor_pk_cw2", STORE_BIN, (2, 8, 8, 64), 64, ACTS_BIN))
    t.append(_case("xnor_pk_cw2", "xnor_pk_cw2", STORE_BIN, (2, 8, 8, 64), 64, ACTS_BIN, "dyadic", "mixed"))
    t.append(_case("xnor_pk_cw2", "xnor_pk_cw2", STORE_BIN, (2, 8, 8, 64), 64, ACTS_BIN, "dyadic", "neg", pool=2))
    t.append(_case("generic", "generic", I4, (2, 10, 20, 24), 24, ACTS_I4_MORE[:5]))
    t.append(_case("generic", "generic", I4, (2, 10, 20, 24), 24, ACTS_I4_MORE[:5], "dyadic", "mixed"))
    t.append(_case("generic", "generic", I4, (2, 10, 20, 24), 24, ACTS_I4, "residual", "mixed", I4, 4, 0.5))
    # ---- the last conv group and the classifier in one launch (qnn_conv2d_dense_forward)
    t.append(_case("mfma_i4_halo64x64", _ps(4, 64), I4, (2, 8, 8, 64), 64, [A(QT, 4, STORE_I4)], pool=2, head=True))
    for sign in ("neg", "mixed"):
        t.append(_case("mfma_i4_halo64x64", _ps(4, 64), I4, (2, 8, 8, 64), 64, [A(QT, 4, STORE_I4)], "dyadic", sign, pool=2,
                       head=True))
    assert len({c["id"] for c in t}) == len(t)
    return t


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _table()
    return _CASES


def head_dense():
    """The classifier of the fused conv + dense cases: 1024 -> 10, 4-bit weights."""
    rng = np.random.default_rng(_seed("head"))
    return {"op": "dense", "kind": "quantized", "nb": 4, "kernel": rng.uniform(-1, 1, (1024, 10)).astype(F32),
            "bias": (rng.standard_normal(10) * 0.1).astype(F32)}
