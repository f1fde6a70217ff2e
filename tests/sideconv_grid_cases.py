"""Depthwise, grouped and transposed convolutions whose pre-activations land exactly on the points where an epilogue can go
wrong, one case per (op, kernel form, epilogue, BN sign): the rounding ties of the three quantised activations, the
threshold of binary_tanh (an exact 0 gives -1), the clip edges, the negative ties of quantized_leakyrelu.  A plain module
(no tests in it), modelled on epilogue_grid_cases.py: test_sideconv_grid_cpu.py proves that every case carries these
points in numbers that are conditions, that they tell a wrong rounding, threshold, clip or per-field constant from the
right one, and that the numpy references of depthwise_cases.py / gconv_cases.py / tconv_cases.py equal the oracle on them;
test_gpu_sideconv_grid.py runs each case on the kernel form it names.

Everything is on a grid (see base()): every intermediate value is a small dyadic number, exact in float32 in any order.

These ops take no shortcut, so the points come from the sums, a bias table and the BN constants: the top-left block of
every image holds one constant code (0; +1 on BIN), so the output pixels whose window lies inside it carry a sum that is the
same in every such pixel (0; on BIN the channel's sum of weights), and the bias of channel ch is chosen so that this sum
lands on target ch mod 7 of the case's activation (targets()): bias = (T - shift) / inv - sum, rounded to a multiple
of 2^-4 (only targets finer than the case's grid are moved by that).  Around these planted points the random part of the map spreads its own.

The expected output comes from oracle/qnn_oracle.py alone: O.quantize / O.binarize / O.ternarize on the whole Keras kernel,
one O.conv2d call per group (depthwise: per channel), concatenated -- for the transposed convolution O.conv2d over the
zero-stuffed, padded input with the flipped kernel --, then O.bias_add, O.batchnorm_inference and the activation
(O.binary_tanh, O.quantized_tanh, O.leaky_relu, and the two functions of qrelu_cases.py, held to golden/ref_qrelu.npz).

What a case claims (claims()): the grid of its pre-activations has the step min(sum step, 2^-4) * min |inv|.  Ties and
the upper clip edge of Q(nb) are odd multiples of 2^-nb, the lower edge region of quantized_relu too, so they are claimed
where that step is <= 2^-nb: always for Q(2) and Q(4); for Q(8) on 8-bit x 8-bit operands (sums step by 2^-8), and behind a
BN on 4-bit operands, float32 input and 8-bit codes x 4-bit weights (2^-6 and 2^-7, times an inv of 1/8) and on BIN / T2
operands (whole-number sums: their Q(8) cases take a BN with inv in 1/128 .. 1/16, bn_of()).  Exempt, WITHOUT BN only:
Q(8) on 4-bit operands, float32 input and 8-bit codes x 4-bit weights (the sums step by 2^-6 and 2^-7: no tie at all) and
on BIN / T2 operands (whole numbers plus a 2^-4 bias).  These cases carry no Q(8) tie, upper-edge or relu-region
requirement; their lower edge, zeros and clipped values are still required.  The negative ties -(10k + 5) / m of quantized_leakyrelu need a step of 2^-(nb-1).
"""
import numpy as np

from oracle import qnn_oracle as O
import epilogue_grid_cases as G
import qact_grid_cases as A
import depthwise_cases as D
import gconv_cases as GC
import tconv_cases as TC

f32 = np.float32
F32, BIN, T2, I4, I8 = D.F32, D.BIN, D.T2, D.I4, D.I8
MIN_TIES, MIN_ZEROS, MIN_EDGE, MIN_DIFF = G.MIN_TIES, G.MIN_ZEROS, G.MIN_EDGE, G.MIN_DIFF
MIN_NEG = 8
NAMES = {F32: "f32", BIN: "bin", T2: "t2", I4: "i4", I8: "i8"}
MOD = {"dw": D, "gc": GC, "tc": TC}
PREFIX = {"dw": "depthwise", "gc": "gconv", "tc": "tconv"}
FN_NAME = {D.FN_NONE: "none", D.FN_LEAKY_RELU: "leaky_relu", D.FN_BINARY_TANH: "binary_tanh",
           D.FN_QUANTIZED_TANH: "quantized_tanh", D.FN_QUANTIZED_RELU: "quantized_relu",
           D.FN_QUANTIZED_LEAKYRELU: "quantized_leakyrelu"}
FN_TAG = {D.FN_NONE: "none", D.FN_LEAKY_RELU: "lrelu", D.FN_BINARY_TANH: "b", D.FN_QUANTIZED_TANH: "q%d",
          D.FN_QUANTIZED_RELU: "relu%d", D.FN_QUANTIZED_LEAKYRELU: "leaky%d"}
POOL1 = dict(pool=1)                       # the wrong_* variants of the two grid modules pool by their case: none here
SIGNS = (None, "pos", "mixed")
# the constant block of every image (rows, columns), and an output pixel whose window lies inside it
BLOCK = {"dw": (4, 6), "gc": (4, 6), "tc": (3, 4)}
MAPS = {"dw": (2, 6, 8), "gc": (2, 6, 8), "tc": (2, 4, 6)}


def form_name(c):
    """The kernel name the entry reports for case c: expected_name of the three GPU test files, restated."""
    s = NAMES[c["store"]]
    if c["store"] not in (I4, I8):
        return "%s_%s" % (PREFIX[c["op"]], s)
    if c["op"] == "dw":
        return "depthwise_%s%s" % (s, "" if D.takes_pk16(c) else "_plain")
    return "%s_%s_%s" % (PREFIX[c["op"]], s, "mfma" if MOD[c["op"]].takes_mfma(c) else "plain")


def flat_pixel(c):
    """An output pixel (y, x) whose taps all read the constant block: (1, 1) of a 3x3 'same' window; for the transposed
    convolution (2, 2), the phase with the most taps (k = 1: (0, 0))."""
    if c["op"] != "tc":
        return 1, 1
    return (2, 2) if c["window"][0] > 1 else (0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# tensors
# ---------------------------------------------------------------------------------------------------------------------
_BASES = {}


def _key(c):
    shape = {"dw": ("C", "M"), "gc": ("Cg", "Fg", "groups"), "tc": ("Cin", "Cout")}[c["op"]]
    return (c["op"], c["store"]) + tuple(c[k] for k in shape) + (c["window"], c["stride"], c["same"], c["map"], c["wkind"],
                                                                c["wbits"], c["x_bits"])


def _conv_sum(c, xv, wq):
    """The oracle's sum of case c: float32 (N, Ho, Wo, cout)."""
    st, pad = (c["stride"], c["stride"]), "same" if c["same"] else "valid"
    if c["op"] == "dw":
        return np.concatenate([O.conv2d(xv[..., ch:ch + 1], wq[:, :, ch:ch + 1, :], st, pad) for ch in range(c["C"])], -1)
    if c["op"] == "gc":
        Cg, Fg = c["Cg"], c["Fg"]
        return np.concatenate([O.conv2d(xv[..., g * Cg:(g + 1) * Cg], wq[..., g * Fg:(g + 1) * Fg], st, pad)
                               for g in range(c["groups"])], -1)
    # transposed: the input with s - 1 zeros between its cells and k - 1 around it, under the kernel turned by 180 degrees
    N, H, W, C = xv.shape
    kh, kw = c["window"]
    s = c["stride"]
    z = np.zeros((N, (H - 1) * s + 1 + 2 * (kh - 1), (W - 1) * s + 1 + 2 * (kw - 1), C), f32)
    z[:, kh - 1:kh + (H - 1) * s:s, kw - 1:kw + (W - 1) * s:s] = xv
    full = O.conv2d(z, np.ascontiguousarray(wq[::-1, ::-1].transpose(0, 1, 3, 2)), (1, 1), "valid")
    return TC.cut(full, s, c["same"], H, W, kh, kw)


def base(c):
    """Input, kernel and the oracle's sum of one (op, store, shape): built once and shared by its epilogues.
    I4: activation codes rint(normal * 2), weight codes -2 .. 2 (sums step by 2^-6).  I8: codes 8 * rint(normal * 2) against
    weight codes +-8 of 8 bits (2^-8) or -2 .. 2 of 4 bits (2^-7: the width the 16-bit-lane depthwise form admits).  BIN:
    +-1 against +-1.  T2: {-1, 0, 1} against ternary weights.  float32: values of the 4-bit grid against 4-bit weights.
    The top-left BLOCK of every image is the constant code.  Returns dict(x: what the entry reads as codes (BIN: 0 / 1) or
    float32 values, xv: float32 values, kernel, wq, v: the sum)."""
    key = _key(c)
    if key in _BASES:
        return _BASES[key]
    rng = np.random.default_rng(G._seed("sideconv", *key))
    op, store = c["op"], c["store"]
    N, H, W = c["map"]
    cin = c["C"] if op == "dw" else c["Cin"]
    kh, kw = c["window"]
    kshape = {"dw": lambda: (kh, kw, c["C"], c["M"]), "gc": lambda: (kh, kw, c["Cg"], c["Cout"]),
              "tc": lambda: (kh, kw, c["Cout"], c["Cin"])}[op]()
    by, bx = BLOCK[op]
    if store == BIN:
        codes = rng.integers(0, 2, (N, H, W, cin))
        codes[:, :by, :bx] = 1
        xv = (2 * codes - 1).astype(f32)
    elif store == T2:
        codes = rng.integers(-1, 2, (N, H, W, cin))
        codes[:, :by, :bx] = 0
        xv = codes.astype(f32)
    else:
        bits = c["x_bits"] or 4
        m = 2 ** (bits - 1)
        codes = np.clip(np.rint(rng.standard_normal((N, H, W, cin)) * 2) * (8 if bits == 8 else 1), -m, m - 1).astype(np.int64)
        codes[:, :by, :bx] = 0
        xv = (codes / m).astype(f32)
    if c["wkind"] == D.W_BINARY:
        kernel = ((rng.integers(0, 2, kshape) * 2 - 1) * 0.5).astype(f32)
        wq = O.binarize(kernel)
        assert np.array_equal(wq, np.sign(kernel))
    elif c["wkind"] == D.W_TERNARY:
        kernel = rng.integers(-1, 2, kshape).astype(f32)
        wq = O.ternarize(kernel)
        assert np.array_equal(wq, kernel)
    else:
        assert c["wkind"] == D.W_QUANT and c["wbits"] in (4, 8)
        wc = rng.integers(-2, 3, kshape) if c["wbits"] == 4 else rng.integers(-1, 2, kshape) * 8
        kernel = (wc / 2.0 ** (c["wbits"] - 1)).astype(f32)
        wq = O.quantize(kernel, c["wbits"])
        assert np.array_equal(wq, kernel)                          # the latent kernel is on the grid
    v = _conv_sum(c, xv, wq)
    y, x = flat_pixel(c)
    assert np.array_equal(v[0, y, x], v[1, y, x])                  # the block's sum, the same in every image
    _BASES[key] = dict(x=xv if store == F32 else codes, xv=xv, kernel=kernel, wq=wq, v=v)
    return _BASES[key]


def sum_step(c):
    """The step of the sums of case c (module docstring)."""
    if c["store"] in (BIN, T2):
        return 1.0
    if c["store"] == I8:
        return 2.0 ** -8 if c["wbits"] == 8 else 2.0 ** -7
    return 2.0 ** -6


_FINE = {}


def bn_of(c):
    """The BN parameters of case c: G.dyadic_bn, inv in 1/8 .. 1.  Q(8) on BIN / T2 operands takes the same parameters with
    gamma / 16 (inv in 1/128 .. 1/16, shift a multiple of 2^-8): whole-number sums plus a 2^-4 bias then step by 2^-11 at
    most and reach the odd multiples of 2^-8, the ties and the upper edge of Q(8)."""
    if c["sign"] is None:
        return None
    n = cout_of(c)
    bn = G.dyadic_bn(n, c["sign"])
    if c["store"] in (BIN, T2) and c["fn"] in D.QACTS and c["act_bits"] == 8:
        if (n, c["sign"]) not in _FINE:
            _FINE[n, c["sign"]] = dict(bn, gamma=(bn["gamma"] / f32(16)).astype(f32))
        bn = _FINE[n, c["sign"]]
    return bn


def cout_of(c):
    return c["C"] * c["M"] if c["op"] == "dw" else c["Cout"]


def constants(c):
    """(inv, shift) as the entry takes them, None without BN."""
    bn = bn_of(c)
    return None if bn is None else O.bn_constants(bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"])


def claims(c, nb, negative=False):
    """Whether the grid of the case's pre-activations holds the ties (negative: the negative ties of quantized_leakyrelu)
    of Q(nb): module docstring."""
    k = constants(c)
    step = min(sum_step(c), 2.0 ** -4) * (1.0 if k is None else float(np.abs(k[0]).min()))
    return step <= 2.0 ** -(nb - 1 if negative else nb)


def targets(c):
    """The seven pre-activation values the bias table aims the block's sum at, by channel mod 7."""
    fn, m = c["fn"], 2.0 ** (c["act_bits"] - 1)
    if fn == D.FN_BINARY_TANH:
        return (0.0, 0.0, 1 / 16, -1 / 16, 0.0, 0.25, -0.25)
    if fn == D.FN_QUANTIZED_TANH:
        return (-1.0, -0.5 / m, 0.5 / m, -1.5 / m, 1.5 / m if m > 2 else 0.5 / m, (m - 1) / m, (m - 0.5) / m)
    if fn == D.FN_QUANTIZED_RELU:
        return (-1 / m, -0.5 / m, 0.0, 0.5 / m, 1.5 / m if m > 2 else 0.75 / m, (m - 1) / m, (m - 0.5) / m)
    if fn == D.FN_QUANTIZED_LEAKYRELU:
        return (-10.0, 0.5 / m, 1.5 / m if m > 2 else 0.5 / m, -5 / m, -15 / m, (m - 1) / m, (m - 0.5) / m)
    return (0.0, 1 / 16, -1 / 16, 0.125, -0.125, 1.0, -1.0)          # FN_NONE, leaky_relu: BIAS8's values


_BIAS = {}


def bias_of(c):
    """The bias table of case c, multiples of 2^-4 (module docstring)."""
    key = (_key(c), c["fn"], c["act_bits"], c["sign"])
    if key not in _BIAS:
        y, x = flat_pixel(c)
        v0 = base(c)["v"][0, y, x].astype(np.float64)
        k = constants(c)
        n = cout_of(c)
        inv, shift = (np.ones(n), np.zeros(n)) if k is None else (k[0].astype(np.float64), k[1].astype(np.float64))
        T = targets(c)
        b = np.empty(n)
        for ch in range(n):
            want = (T[ch % 7] - shift[ch]) / inv[ch] - v0[ch]
            want = np.rint(want * 16) / 16
            b[ch] = want
        assert np.array_equal(b * 16, np.rint(b * 16)) and np.abs(b).max() < 2048
        _BIAS[key] = b.astype(f32)
    return _BIAS[key]


def preactivation(c, perm=None):
    """The oracle's float32 value the activation is applied to.  perm: the channel whose bias and BN constants channel ch
    takes (the per-field mix-up)."""
    n = cout_of(c)
    perm = np.arange(n) if perm is None else perm
    p = O.bias_add(base(c)["v"], bias_of(c)[perm])
    bn = bn_of(c)
    if bn is not None:
        p = O.batchnorm_inference(p, bn["gamma"][perm], bn["beta"][perm], bn["mean"][perm], bn["var"][perm], bn["eps"])
    return p


def activate(c, p):
    fn = c["fn"]
    if fn == D.FN_NONE:
        return np.asarray(p, f32)
    if fn == D.FN_LEAKY_RELU:
        return O.leaky_relu(p)
    return G.ACT[FN_NAME[fn]](p, c["act_bits"])


def expected(c, p=None):
    """The oracle's output of case c as float32 values."""
    return activate(c, preactivation(c) if p is None else p)


def stored(c, y):
    """Float32 values y as the out_store of case c holds them, in the form D.reference returns: the values themselves, the
    bit of a BIN output, else the integer codes."""
    if c["out_store"] == F32:
        return y
    if c["fn"] == D.FN_BINARY_TANH:
        assert np.all(np.abs(y) == 1)
        return (y > 0).astype(np.int64) if c["out_store"] == BIN else y.astype(np.int64)
    return O.codes_of(y, c["act_bits"])


# ---------------------------------------------------------------------------------------------------------------------
# what a case must carry, counted on the pre-activation, and the wrong epilogues it must tell from the right one
# ---------------------------------------------------------------------------------------------------------------------
def _region(t, values):
    n = [int(np.count_nonzero(t == x)) for x in values]
    return sum(n) if min(n) else 0


def counts(c, p):
    """dict(ties, neg, zeros, lo, hi) of pre-activation p under the case's activation: ties strictly inside the clip range;
    the negative ties of quantized_leakyrelu; exact zeros; points on the lower edge (t = -m; quantized_relu: the region
    -1, -1/2, 0, 1/2, each of which must occur) and in the upper edge region (m - 1 and m - 1/2, both must occur)."""
    fn, nb = c["fn"], c["act_bits"]
    out = dict(zeros=G.zero_count(p))
    if fn not in D.QACTS:
        return out
    m = 2.0 ** (nb - 1)
    t, off, lo_clip = _t_off_lo(c, p)
    t = t - off
    out["ties"] = int(np.count_nonzero((t - np.floor(t) == 0.5) & (t > lo_clip) & (t < m - 1)))
    out["hi"] = _region(t, (m - 1, m - 0.5))
    out["lo"] = _region(t, (-1.0, -0.5, 0.0, 0.5)) if fn == D.FN_QUANTIZED_RELU else int(np.count_nonzero(t == -m))
    out["beyond"] = int(np.count_nonzero((t < lo_clip - 0.5) | (t > m - 0.5)))
    if fn == D.FN_QUANTIZED_LEAKYRELU:
        out["neg"] = A.neg_tie_count(p, nb)
    return out


def _t_off_lo(c, p):
    fn, nb = c["fn"], c["act_bits"]
    if fn == D.FN_QUANTIZED_TANH:
        return p.astype(np.float64) * 2.0 ** (nb - 1), 0.0, -(2.0 ** (nb - 1))
    return A._t(p, FN_NAME[fn], nb)


def swap_fields(c):
    """The per-field mix-up: channel ch takes the constants of channel ch ^ 1 (the last of an odd count keeps its own)."""
    n = cout_of(c)
    return np.minimum(np.arange(n) ^ 1, n - 1)


def wrong(c, p):
    """name -> the output of a wrong epilogue on pre-activation p, as float32 values."""
    fn, nb = c["fn"], c["act_bits"]
    out = {"fields": expected(c, preactivation(c, swap_fields(c)))}
    if fn == D.FN_BINARY_TANH:
        out["ge0"] = G.wrong_binary_ge0(POOL1, p)
    if fn in D.QACTS:
        m = 2.0 ** (nb - 1)
        t, off, lo = _t_off_lo(c, p)
        if fn == D.FN_QUANTIZED_TANH:
            out["half_away"], out["half_up"] = G.wrong_half_away(POOL1, p, nb), G.wrong_floor_half(POOL1, p, nb)
        else:
            out["half_away"] = A.wrong_half_away(POOL1, p, FN_NAME[fn], nb)
            out["half_up"] = A.wrong_floor_half(POOL1, p, FN_NAME[fn], nb)
        out["trunc"] = (np.clip(np.trunc(t) - off, lo, m - 1) / m).astype(f32)
        out["clip_m"] = (np.clip(np.rint(t) - off, lo, m) / m).astype(f32)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
ALL_OUT = (F32, BIN, I4, I8)


def epilogues(outs):
    """(fn, act_bits, out_store) of a form that stores to `outs`: binary_tanh to every store, the three quantised
    activations at 2, 4 and 8 bits where the store holds them, FN_NONE and leaky_relu to float32."""
    e = []
    for os in outs:
        e.append((D.FN_BINARY_TANH, 0, os))
        if os != BIN:
            e += [(fn, nb, os) for fn in D.QACTS for nb in (2, 4, 8) if os == F32 or nb <= os]
        if os == F32:
            e += [(D.FN_NONE, 0, F32), (D.FN_LEAKY_RELU, 0, F32)]
    return e


def _wk(store, wbits=None):
    if store == BIN:
        return dict(wkind=D.W_BINARY, wbits=1, x_bits=1)
    if store == T2:
        return dict(wkind=D.W_TERNARY, wbits=1, x_bits=1)
    if store == F32:
        return dict(wkind=D.W_QUANT, wbits=4, x_bits=0)
    return dict(wkind=D.W_QUANT, wbits=wbits or store, x_bits=store)


def _forms():
    """(op, form, tag, shape of the op's _case, out_stores).  A fast form stores to its own store only; the same codes
    written to every other store take the plain form (the twin of test_gpu_sideconv_grid.py)."""
    f = []
    other = lambda s: tuple(o for o in ALL_OUT if o != s)          # noqa: E731
    # ---- depthwise: C = 33 (a ragged last int4 word) and 16 (all fields of every int8 word); 4-bit weights keep the 8-bit
    # codes inside the 16-bit bound, 8-bit weights leave it
    f.append(("dw", "depthwise_i4", "C33", dict(store=I4, C=33, **_wk(I4)), (I4,)))
    f.append(("dw", "depthwise_i4_plain", "C33", dict(store=I4, C=33, **_wk(I4)), other(I4)))
    f.append(("dw", "depthwise_i4_plain", "C17M2", dict(store=I4, C=17, M=2, **_wk(I4)), ALL_OUT))
    f.append(("dw", "depthwise_i8", "C16w4", dict(store=I8, C=16, **_wk(I8, 4)), (I8,)))
    f.append(("dw", "depthwise_i8_plain", "C16w4", dict(store=I8, C=16, **_wk(I8, 4)), other(I8)))
    f.append(("dw", "depthwise_i8_plain", "C16w8", dict(store=I8, C=16, **_wk(I8)), ALL_OUT))
    f.append(("dw", "depthwise_i8_plain", "C8M2w4", dict(store=I8, C=8, M=2, **_wk(I8, 4)), (I8,)))
    f.append(("dw", "depthwise_bin", "C33", dict(store=BIN, C=33, **_wk(BIN)), ALL_OUT))
    f.append(("dw", "depthwise_t2", "C33", dict(store=T2, C=33, **_wk(T2)), ALL_OUT))
    f.append(("dw", "depthwise_f32", "C16", dict(store=F32, C=16, **_wk(F32)), ALL_OUT))
    # ---- grouped: (Cg, Fg, g) = (4, 4, 4), the smallest the route rule admits (Cout = 16, runs of 16 channels); (3, 6, 3)
    # and (5, 6, 3) miss it (Cout = 18)
    for s in (I4, I8):
        n = NAMES[s]
        f.append(("gc", "gconv_%s_mfma" % n, "4x4g4", dict(store=s, Cg=4, Fg=4, groups=4, **_wk(s)), (s,)))
        f.append(("gc", "gconv_%s_plain" % n, "4x4g4", dict(store=s, Cg=4, Fg=4, groups=4, **_wk(s)), other(s)))
        f.append(("gc", "gconv_%s_plain" % n, "3x6g3", dict(store=s, Cg=3, Fg=6, groups=3, **_wk(s)), ALL_OUT))
    for s in (BIN, T2):
        f.append(("gc", "gconv_" + NAMES[s], "5x6g3", dict(store=s, Cg=5, Fg=6, groups=3, **_wk(s)), ALL_OUT))
    f.append(("gc", "gconv_f32", "3x6g3", dict(store=F32, Cg=3, Fg=6, groups=3, **_wk(F32)), ALL_OUT))
    # ---- transposed, 3x3 at stride 2 (phases of 4, 2, 2 and 1 taps, all inside the constant block): 64 -> 16 is the
    # smallest the route rule admits; 9 -> 18 and 33 -> 18 miss it.  1x1 at stride 2: three outputs of four see no tap.
    for s in (I4, I8):
        n = NAMES[s]
        f.append(("tc", "tconv_%s_mfma" % n, "64to16", dict(store=s, Cin=64, Cout=16, **_wk(s)), (s,)))
        f.append(("tc", "tconv_%s_plain" % n, "64to16", dict(store=s, Cin=64, Cout=16, **_wk(s)), other(s)))
        f.append(("tc", "tconv_%s_plain" % n, "9to18", dict(store=s, Cin=9, Cout=18, **_wk(s)), ALL_OUT))
    f.append(("tc", "tconv_i4_plain", "9to18k1", dict(store=I4, Cin=9, Cout=18, window=(1, 1), **_wk(I4)), ALL_OUT))
    for s in (BIN, T2):
        f.append(("tc", "tconv_" + NAMES[s], "33to18", dict(store=s, Cin=33, Cout=18, **_wk(s)), ALL_OUT))
    f.append(("tc", "tconv_f32", "9to18", dict(store=F32, Cin=9, Cout=18, **_wk(F32)), ALL_OUT))
    return f


def _make(op, shape, fn, nb, os, sign):
    kw = dict(shape)
    store = kw.pop("store")
    extra = dict(fn=fn, act_bits=nb, out_store=os, bias=True, bn=sign is not None, map=MAPS[op], **kw)
    if op == "dw":
        c = D._case(store, extra.pop("C"), **extra)
    elif op == "gc":
        c = GC._case(store, extra.pop("Cg"), extra.pop("Fg"), extra.pop("groups"), **extra)
    else:
        c = TC._case(store, extra.pop("Cin"), extra.pop("Cout"), **extra)
    c.setdefault("dil", (1, 1))
    c.update(op=op, sign=sign)
    return c


def _table():
    t = []
    for op, form, tag, shape, outs in _forms():
        for fn, nb, os in epilogues(outs):
            for sign in SIGNS:
                c = _make(op, shape, fn, nb, os, sign)
                c["form"] = form
                c["id"] = "-".join((form, tag, FN_TAG[fn].replace("%d", str(nb)), NAMES[os], sign or "nobn"))
                t.append(c)
    assert len({c["id"] for c in t}) == len(t)
    return t


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _table()
    return _CASES


def groups(op=None):
    """The (op, form, tag) groups of the table in its order (one per line of _forms()); `op`: those of one op."""
    seen = []
    for c in cases():
        g = (c["op"], c["form"], c["id"].split("-")[1])
        if g not in seen and op in (None, c["op"]):
            seen.append(g)
    return seen


def group_cases(g):
    return [c for c in cases() if (c["op"], c["form"], c["id"].split("-")[1]) == g]


def hosted(op, host_stores):
    """The groups of `op` by hosting test id: host_stores is the input store of each test_epilogues id of the op's GPU file, in
    order; a group goes to the host of its own input store that carries the fewest groups (the first of them).  Returns
    one list of groups per host."""
    out = [[] for _ in host_stores]
    for g in groups(op):
        store = group_cases(g)[0]["store"]
        k = min((i for i, s_ in enumerate(host_stores) if s_ == store), key=lambda i: (len(out[i]), i))
        out[k].append(g)
    return out


def twin(c):
    """The plain-form case on the same codes as fast-form case c (None for a plain case): the same layer and epilogue
    written to the other packed store, or to float32 where that store does not hold the activation's width."""
    if not (c["form"].endswith("_mfma") or c["form"] in ("depthwise_i4", "depthwise_i8")):
        return None
    os = I8 if c["store"] == I4 else (I4 if c["act_bits"] <= 4 else F32)
    tag = c["id"].split("-")[1]
    form = "%s_%s_plain" % (PREFIX[c["op"]], NAMES[c["store"]])
    return next(k for k in cases() if k["form"] == form and k["id"].split("-")[1] == tag and k["sign"] == c["sign"] and
                (k["fn"], k["act_bits"], k["out_store"]) == (c["fn"], c["act_bits"], os))


def inputs(c):
    """(x, kernel, bias, (inv, shift) or None) as reference() of the op's case module and the GPU harness take them."""
    b = base(c)
    return b["x"], b["kernel"], bias_of(c), constants(c)
