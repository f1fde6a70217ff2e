"""Cases and a numpy reference for the depthwise convolution (include/qnn_abi_depthwise.h).

The reference restates, in numpy float32 / int64 / float64, what the entry promises: the weight quantisers applied
elementwise to the Keras kernel (kh, kw, C, M), the exact integer sum over the in-bounds taps (float32 input: a float64
sum in (ky, kx) row-major order, rounded once), the float32 chain bias -> BN -> activation in the reference's op order,
and the encoding of the stores.  Nothing here imports the package under test.
"""
import itertools

import numpy as np

F32, BIN, T2, I4, I8 = 0, 1, 2, 4, 8
W_FLOAT, W_BINARY, W_QUANT, W_TERNARY = 0, 1, 2, 3
FN_NONE, FN_BINARY_TANH, FN_QUANTIZED_TANH, FN_LEAKY_RELU, FN_QUANTIZED_RELU, FN_QUANTIZED_LEAKYRELU = 0, 1, 2, 5, 6, 7
QACTS = (FN_QUANTIZED_TANH, FN_QUANTIZED_RELU, FN_QUANTIZED_LEAKYRELU)
f32 = np.float32


# ---- geometry (csrc/qnn_conv_geom.h) ------------------------------------------------------------------------------------
def out_pad(size, k, s, same, d=1):
    """(out, pad_before) of one axis on the effective window d * (k - 1) + 1."""
    ke = d * (k - 1) + 1
    if same:
        out = -(-size // s)
        return out, max((out - 1) * s + ke - size, 0) // 2
    return ((size - ke) // s + 1 if size >= ke else 0), 0


# ---- weight quantisers ---------------------------------------------------------------------------------------------------
def binary_tanh(x):
    x = np.asarray(x, f32)
    h = np.clip(f32(0.5) * x + f32(0.5), f32(0), f32(1)).astype(f32)
    r = np.rint(h).astype(f32)
    rt = (h + (r - h)).astype(f32)
    return (f32(2) * rt - f32(1)).astype(f32)


def quantize_weights(kernel, wkind, wbits=0, H=1.0):
    """(quantized float32 values, integer codes, wshift); codes = values * 2^wshift (None for float weights)."""
    k = np.asarray(kernel, f32)
    H = f32(H)
    if wkind == W_FLOAT:
        return k, None, 0
    if wkind == W_BINARY:
        q = (H * binary_tanh(k / H)).astype(f32)
        return q, np.rint(q).astype(np.int64), 0
    if wkind == W_QUANT:
        m = f32(2 ** (wbits - 1))
        t = (k * m).astype(f32)
        r = np.rint(t).astype(f32)
        code = np.clip((t + (r - t)).astype(f32), -m, m - f32(1))
        return (code * (f32(1) / m)).astype(f32), code.astype(np.int64), wbits - 1
    u = (k / H).astype(f32)
    cutoff = f32(0.7) * f32(np.abs(u).astype(np.float64).sum() / u.size)
    t = np.where(u > cutoff, f32(1), np.where(u <= -cutoff, f32(-1), f32(0))).astype(f32)
    q = (t * H).astype(f32)
    return q, np.rint(q).astype(np.int64), 0


# ---- the convolution -------------------------------------------------------------------------------------------------------
def dw_sum(x, w, stride, same, dil=(1, 1), dtype=np.int64):
    """sum over the in-bounds taps of x[n, y, x, c] * w[ky, kx, c, m] -> (N, Ho, Wo, C * M), accumulated in `dtype` in
    (ky, kx) row-major order.  A tap outside the image adds nothing (a zero product leaves both kinds of sum unchanged)."""
    N, H, W, C = x.shape
    kh, kw, _, M = w.shape
    Ho, pt = out_pad(H, kh, stride, same, dil[0])
    Wo, pl = out_pad(W, kw, stride, same, dil[1])
    acc = np.zeros((N, Ho, Wo, C, M), dtype)
    xs, ws = x.astype(dtype), w.astype(dtype)
    for ky in range(kh):
        for kx in range(kw):
            for oy in range(Ho):
                yy = oy * stride - pt + ky * dil[0]
                if not 0 <= yy < H:
                    continue
                for ox in range(Wo):
                    xx = ox * stride - pl + kx * dil[1]
                    if 0 <= xx < W:
                        acc[:, oy, ox] += xs[:, yy, xx, :, None] * ws[ky, kx][None]
    return acc.reshape(N, Ho, Wo, C * M)


def expand_block_diagonal(kernel):
    """Keras depthwise kernel (kh, kw, C, M) -> the full HWIO kernel (kh, kw, C, C * M) that is zero off the diagonal."""
    kh, kw, C, M = kernel.shape
    full = np.zeros((kh, kw, C, C * M), kernel.dtype)
    for c in range(C):
        full[:, :, c, c * M:(c + 1) * M] = kernel[:, :, c, :]
    return full


def takes_pk16(c):
    """The host's rule for the 16-bit-lane form, restated: depth_multiplier 1, 3x3 at stride 1 without dilation, I4 / I8
    codes in and out, and the bound."""
    wshift = c["wbits"] - 1 if c["wkind"] == W_QUANT else 0
    return (c["store"] in (I4, I8) and c["out_store"] == c["store"] and c["M"] == 1 and c["window"] == (3, 3) and
            c["stride"] == 1 and c["dil"] == (1, 1) and pk16_bound_ok(3, 3, c["x_bits"], wshift))


def pk16_bound_ok(kh, kw, x_bits, wshift):
    """kh * kw * 2^(x_bits-1) * 2^wshift < 2^15: no partial sum of the taps leaves a signed 16-bit lane."""
    return kh * kw * (1 << (x_bits - 1)) * (1 << wshift) < (1 << 15)


# ---- the float32 chain -----------------------------------------------------------------------------------------------------
def qact_code(fn, v, m):
    v = np.asarray(v, f32)
    m = f32(m)
    if fn == FN_QUANTIZED_RELU:
        r = (np.rint(((v + f32(1)).astype(f32) * m).astype(f32)) - m).astype(f32)
        return np.clip(r, f32(0), m - f32(1)).astype(f32)
    if fn == FN_QUANTIZED_LEAKYRELU:
        v = np.where(v >= 0, v, (f32(0.1) * v).astype(f32)).astype(f32)
    t = (v * m).astype(f32)
    r = np.rint(t).astype(f32)
    return np.clip((t + (r - t)).astype(f32), -m, m - f32(1)).astype(f32)


def chain(v, bias, bn, fn, act_bits, out_store):
    """v float32 (..., cout) -> float32 values (out_store F32) or integer codes (BIN: 0 / 1)."""
    v = np.asarray(v, f32)
    if bias is not None:
        v = (v + bias.astype(f32)).astype(f32)
    if bn is not None:
        v = ((v * bn[0].astype(f32)).astype(f32) + bn[1].astype(f32)).astype(f32)
    m = f32(2 ** (act_bits - 1)) if fn in QACTS else f32(1)
    if out_store == F32:
        if fn == FN_BINARY_TANH:
            return binary_tanh(v)
        if fn in QACTS:
            return (qact_code(fn, v, m) * (f32(1) / m)).astype(f32)
        if fn == FN_LEAKY_RELU:
            return np.where(v >= 0, v, (v * f32(0.3)).astype(f32)).astype(f32)
        return v
    if fn == FN_BINARY_TANH:
        bit = (binary_tanh(v) > 0).astype(np.int64)
        return bit if out_store == BIN else 2 * bit - 1
    return qact_code(fn, v, m).astype(np.int64)


# ---- the stores ------------------------------------------------------------------------------------------------------------
def per_word(store):
    return {BIN: 32, T2: 32, I4: 8, I8: 4}[store]


def words(store, C):
    return 2 * (-(-C // 32)) if store == T2 else -(-C // per_word(store))


def encode(codes, store, spare=None):
    """codes (..., C) integers (BIN: 0 / 1; T2: -1 / 0 / 1) -> uint32 words (..., words).  spare: a RandomState that fills
    the bits beyond channel C - 1 of the last word (T2: of both planes) with noise, or None = zero."""
    codes = np.asarray(codes, np.int64)
    C = codes.shape[-1]
    lead = codes.shape[:-1]
    if store == T2:
        nw = -(-C // 32)
        full = np.zeros(lead + (nw * 32,), np.int64)
        full[..., :C] = codes
        mask, sign = (full != 0).astype(np.uint64), (full > 0).astype(np.uint64)
        if spare is not None:
            mask[..., C:] = spare.randint(0, 2, lead + (nw * 32 - C,))
            sign[..., C:] = spare.randint(0, 2, lead + (nw * 32 - C,))
        sh = np.arange(32, dtype=np.uint64)
        mw = (mask.reshape(lead + (nw, 32)) << sh).sum(-1)
        sw = (sign.reshape(lead + (nw, 32)) << sh).sum(-1)
        return np.stack([mw, sw], -1).reshape(lead + (2 * nw,)).astype(np.uint32)
    pw = per_word(store)
    bits = 32 // pw
    nw = -(-C // pw)
    full = np.zeros(lead + (nw * pw,), np.int64)
    full[..., :C] = codes
    if spare is not None:
        full[..., C:] = spare.randint(0, 1 << bits, lead + (nw * pw - C,))
    fields = (full & ((1 << bits) - 1)).astype(np.uint64).reshape(lead + (nw, pw))
    return (fields << (np.arange(pw, dtype=np.uint64) * np.uint64(bits))).sum(-1).astype(np.uint32)


def decode(wordsarr, store, C):
    """uint32 words (..., words) -> (codes (..., C) int64 with BIN as 0 / 1, the spare bits of the last word as int)."""
    w = np.asarray(wordsarr).astype(np.uint64)
    pw = per_word(store)
    bits = 32 // pw
    f = (w[..., :, None] >> (np.arange(pw, dtype=np.uint64) * np.uint64(bits))) & np.uint64((1 << bits) - 1)
    f = f.reshape(w.shape[:-1] + (-1,)).astype(np.int64)
    if store != BIN:
        f = np.where(f >= (1 << (bits - 1)), f - (1 << bits), f)
    return f[..., :C], f[..., C:]


def values_of(codes, store, bits):
    """float32 values of input codes: BIN 0 / 1 -> -1 / +1; T2 as is; I4 / I8 code / 2^(bits-1)."""
    c = np.asarray(codes, np.int64)
    if store == BIN:
        return (2 * c - 1).astype(f32)
    if store == T2:
        return c.astype(f32)
    return (c.astype(f32) * f32(2.0 ** -(bits - 1))).astype(f32)


def signed_codes(codes, store):
    return 2 * np.asarray(codes, np.int64) - 1 if store == BIN else np.asarray(codes, np.int64)


def random_codes(rs, shape, store, bits):
    if store == BIN:
        return rs.randint(0, 2, shape)
    if store == T2:
        return rs.randint(-1, 2, shape)
    return rs.randint(-(1 << (bits - 1)), 1 << (bits - 1), shape)


def reference(case, x_codes_or_f32, kernel, bias, bn):
    """The expected output of one case: float32 values or integer codes, shaped (N, Ho, Wo, C * M)."""
    q, wcode, wshift = quantize_weights(kernel, case["wkind"], case.get("wbits", 0))
    if case["store"] == F32:
        v = dw_sum(np.asarray(x_codes_or_f32, f32), q, case["stride"], case["same"], case["dil"], np.float64).astype(f32)
    else:
        acc = dw_sum(signed_codes(x_codes_or_f32, case["store"]), wcode, case["stride"], case["same"], case["dil"])
        xshift = case["x_bits"] - 1 if case["store"] in (I4, I8) else 0
        v = (acc.astype(f32) * f32(2.0 ** -(wshift + xshift))).astype(f32)
    return chain(v, bias, bn, case["fn"], case.get("act_bits", 0), case["out_store"])


# ---- the case table ------------------------------------------------------------------------------------------------------
CHANNELS = {I4: (1, 7, 8, 9, 32, 33), I8: (3, 4, 5, 16), BIN: (31, 32, 33, 128), T2: (33, 64), F32: (1, 5)}
WINDOWS = ((1, 1), (3, 3), (2, 3), (5, 5))
MAP = (2, 5, 7)          # N, H, W
SMALL_MAP = (2, 2, 2)    # smaller than the window under 'same'


def _case(store, C, **kw):
    c = dict(store=store, C=C, M=1, window=(3, 3), stride=1, same=True, dil=(1, 1), map=MAP, bias=True, bn=True,
             misalign=False)
    if store == F32:
        c.update(wkind=W_FLOAT, wbits=0, x_bits=0, fn=FN_NONE, act_bits=0, out_store=F32)
    elif store == BIN:
        c.update(wkind=W_BINARY, wbits=1, x_bits=1, fn=FN_BINARY_TANH, act_bits=0, out_store=BIN)
    elif store == T2:
        c.update(wkind=W_TERNARY, wbits=1, x_bits=1, fn=FN_QUANTIZED_TANH, act_bits=4, out_store=I4)
    else:
        c.update(wkind=W_QUANT, wbits=store, x_bits=store, fn=FN_QUANTIZED_TANH, act_bits=store, out_store=store)
    c.update(kw)
    return c


def case_id(c):
    return "s%d_C%d_M%d_k%dx%d_s%d_%s_d%dx%d_w%d.%d_x%d_fn%d.%d_o%d_%s%s%s_%s" % (
        c["store"], c["C"], c["M"], c["window"][0], c["window"][1], c["stride"], "same" if c["same"] else "valid",
        c["dil"][0], c["dil"][1], c["wkind"], c["wbits"], c["x_bits"], c["fn"], c["act_bits"], c["out_store"],
        "b" if c["bias"] else "", "n" if c["bn"] else "", "m" if c["misalign"] else "", "x".join(map(str, c["map"])))


def geometry_cases():
    """Every store and channel count at 3x3 'same'; the widest of each store also 4 bytes off alignment; every window,
    stride, padding, dilation and depth multiplier on one count per store; the 2x2 map."""
    out = []
    for store, chans in CHANNELS.items():
        for C in chans:
            out.append(_case(store, C))
        out.append(_case(store, max(chans), misalign=True))
        C = chans[1]
        for window, stride, same in itertools.product(WINDOWS, (1, 2), (True, False)):
            if (window, stride, same) != ((3, 3), 1, True):
                out.append(_case(store, C, window=window, stride=stride, same=same))
        for dil in ((2, 2), (1, 2)):
            out.append(_case(store, C, dil=dil))
            out.append(_case(store, C, dil=dil, same=False, window=(2, 3)))
        for M in (2, 3):
            out.append(_case(store, C, M=M))
            out.append(_case(store, max(chans), M=M, window=(2, 3), stride=2))
        out.append(_case(store, C, map=SMALL_MAP))
        out.append(_case(store, max(chans), map=SMALL_MAP, window=(5, 5)))
        for stride in (1, 2):                # the widest window the entry takes (QNN_DW_MAX_WINDOW)
            out.append(_case(store, C, window=(7, 7), stride=stride))
        out.append(_case(store, chans[0], window=(7, 7), same=False, map=(1, 8, 9)))
    return out


def weight_cases():
    """Each weight kind on each store whose rules allow it (qnn_depthwise_prepack)."""
    out = []
    for store, C in ((I4, 9), (I8, 5)):
        for wkind, wbits in ((W_BINARY, 1), (W_TERNARY, 1), (W_QUANT, 2), (W_QUANT, 4), (W_QUANT, 8)):
            if wkind == W_QUANT and wbits > store:
                continue
            for x_bits in sorted({2, 4, store}):
                out.append(_case(store, C, wkind=wkind, wbits=wbits, x_bits=x_bits))
    out.append(_case(T2, 33, wkind=W_BINARY))
    for wkind, wbits in ((W_BINARY, 1), (W_TERNARY, 1), (W_QUANT, 2), (W_QUANT, 4), (W_QUANT, 8), (W_QUANT, 16)):
        out.append(_case(F32, 5, wkind=wkind, wbits=wbits))
    return out


def epilogue_cases():
    """Each supported fn to each legal out_store, with and without BN and bias, on the plain and the 16-bit-lane form."""
    out = []
    for store, C, M in ((I4, 33, 1), (I8, 16, 1), (I4, 9, 2), (BIN, 33, 1), (T2, 33, 1), (F32, 5, 1)):
        pairs = [(FN_NONE, 0, F32), (FN_LEAKY_RELU, 0, F32), (FN_BINARY_TANH, 0, F32), (FN_BINARY_TANH, 0, BIN),
                 (FN_BINARY_TANH, 0, I4), (FN_BINARY_TANH, 0, I8)]
        for fn in QACTS:
            pairs += [(fn, 4, F32), (fn, 2, I4), (fn, 4, I4), (fn, 4, I8), (fn, 6, I8), (fn, 8, I8)]
        for (fn, ab, os), (bias, bn) in itertools.product(pairs, ((True, True), (False, False))):
            out.append(_case(store, C, M=M, fn=fn, act_bits=ab, out_store=os, bias=bias, bn=bn))
        out.append(_case(store, C, M=M, bias=True, bn=False))
        out.append(_case(store, C, M=M, bias=False, bn=True))
    return out


def bound_cases():
    """Both sides of the 16-bit bound at 3x3: 4/4 and 8-bit codes x 4-bit weights inside, 8/8 outside."""
    return [_case(I4, 32, wbits=4, x_bits=4), _case(I8, 16, wbits=4, x_bits=8), _case(I8, 16, wbits=8, x_bits=4),
            _case(I8, 16, wbits=8, x_bits=8), _case(I8, 16, wbits=7, x_bits=6), _case(I8, 16, wbits=7, x_bits=7)]


def make_inputs(c, seed=0):
    """Deterministic inputs of a case: (x codes or float32 values, kernel (kh, kw, C, M), bias or None, (inv, shift) or
    None).  Kernel values are multiples of 1/64 in [-1, 1] (the ternary cutoff's float64 mean is then exact in any order);
    bias and BN constants are small dyadic numbers, so pre-activations land on rounding ties and clip edges."""
    rs = np.random.RandomState(1000 + seed)
    N, H, W = c["map"]
    C, M = c["C"], c["M"]
    kh, kw = c["window"]
    if c["store"] == F32:
        x = (rs.randint(-64, 65, (N, H, W, C)) / 32.0).astype(f32) + (rs.rand(N, H, W, C) < 0.3) * f32(1e-3)
        x = x.astype(f32)
    else:
        x = random_codes(rs, (N, H, W, C), c["store"], c["x_bits"])
    kernel = (rs.randint(-64, 65, (kh, kw, C, M)) / 64.0).astype(f32)
    bias = (rs.randint(-8, 9, C * M) / 16.0).astype(f32) if c["bias"] else None
    bn = None
    if c["bn"]:
        bn = ((2.0 ** rs.randint(-2, 2, C * M)).astype(f32) * rs.choice([-1, 1], C * M).astype(f32),
              (rs.randint(-8, 9, C * M) / 32.0).astype(f32))
    return x, kernel, bias, bn


# ---- maps on which a kernel's item decode is not trivial ---------------------------------------------------------------------
K_ROWS = 4               # output rows an item of k_dw_pk16 walks (csrc/qnn_depthwise.hip)
BLOCK = 256              # lanes of a workgroup of every kernel of the three side convolutions
TINY_MAP = (70, 1, 1)    # more images than a workgroup has waves, one pixel each


def pk16_items(c):
    """(row blocks per image, rows of the last one, items) of k_dw_pk16's launch: an item is (image, block of K_ROWS output
    rows, output column, word), the word fastest."""
    N, H, W = c["map"]
    Ho = out_pad(H, 3, 1, c["same"])[0]
    Wo = out_pad(W, 3, 1, c["same"])[0]
    blocks = -(-Ho // K_ROWS)
    return blocks, Ho - (blocks - 1) * K_ROWS, N * blocks * Wo * words(c["store"], c["C"])


def plain_items(out_store, cout, pixels, misalign):
    """(V, items) of a plain-form launch of the three side convolutions: a lane owns V = 4 words (float32: channels) of one
    output pixel where the words per pixel divide by 4 and the pointers are 16-byte aligned, V = 1 otherwise."""
    ocw = cout if out_store == F32 else words(out_store, cout)
    V = 4 if ocw % 4 == 0 and not misalign else 1
    return V, pixels * (ocw // V)


def clip_ends(c):
    """(lowest, highest) output of a case's activation as `reference` returns it; None where nothing clips."""
    if c["fn"] in QACTS:
        m = 2 ** (c["act_bits"] - 1)
        lo = 0 if c["fn"] == FN_QUANTIZED_RELU else -m
        return (lo, m - 1) if c["out_store"] != F32 else (f32(lo) / f32(m), f32(m - 1) / f32(m))
    if c["fn"] == FN_BINARY_TANH:
        return (0, 1) if c["out_store"] == BIN else (-1, 1)
    return None


def degenerate(c, want, groups=None):
    """Why the expected output `want` (N, Ho, Wo, cout) of case `c` could not tell one pixel mapping from another, as a list
    of sentences (empty: it can).  More than half of the outputs at the activation's two clip ends (a 1-bit output has no
    other code: there the rarer code must hold a quarter); two images with equal outputs; two 16-pixel groups of an image
    with equal outputs, a ragged last group compared over its own pixels.  `groups`: per image the groups as arrays
    (pixels, cout); the default cuts the flattened map into 16-pixel runs."""
    why = []
    N = want.shape[0]
    ends = clip_ends(c)
    if ends is not None:
        lo, hi = np.mean(want == ends[0]), np.mean(want == ends[1])
        if c["out_store"] == BIN or c["fn"] == FN_BINARY_TANH:
            if min(lo, hi) < 0.25:
                why.append("one of the two codes holds %.3f of the outputs" % min(lo, hi))
        elif lo + hi > 0.5:
            why.append("%.3f of the outputs sit at a clip end" % (lo + hi))
    flat = want.reshape(N, -1, want.shape[-1])
    for a, b in itertools.combinations(range(N), 2):
        if np.array_equal(flat[a], flat[b]):
            why.append("images %d and %d are equal" % (a, b))
    for n in range(N):
        gs = groups[n] if groups is not None else [flat[n, i:i + 16] for i in range(0, flat.shape[1], 16)]
        for (i, a), (j, b) in itertools.combinations(enumerate(gs), 2):
            k = min(len(a), len(b))
            if k and np.array_equal(a[:k], b[:k]):
                why.append("image %d: groups %d and %d are equal" % (n, i, j))
    return why


def multitask_cases():
    """Maps on which k_dw_pk16's item decode (image, row block, column, word) and the plain form's (pixel, word group) leave
    the first workgroup and the first row block.  Every case carries the `seed` of its inputs.
    pk16, I4 C = 33 (5 words) and I8 C = 16 (4 words; 4-bit weights keep the 16-bit bound) with 4-bit outputs, so that the
    other packed store takes the same codes through the plain form:
      (3, 10, 9)  3 row blocks, the last with 2 rows; 405 and 324 items: a second workgroup, partly filled
      (2, 8, 17)  Ho % 4 == 0: no ragged row block; 340 and 272 items
      (2, 13, 5)  4 row blocks, the last with 1 row
      TINY_MAP    I4 only: 350 items, the image index runs to 69
    plain form, BIN C = 256 (8 words) on (2, 9, 9): 324 items at V = 4, and off alignment 1296 at V = 1."""
    out = []
    for store, C, kw in ((I4, 33, {}), (I8, 16, dict(wbits=4))):
        for m in ((3, 10, 9), (2, 8, 17), (2, 13, 5)):
            out.append(_case(store, C, map=m, act_bits=4, seed=0, **kw))
    out.append(_case(I4, 33, map=TINY_MAP, seed=0))
    for misalign in (False, True):
        out.append(_case(BIN, 256, map=(2, 9, 9), misalign=misalign, seed=0))
    return out


def overflow_case():
    """3x3, 8-bit codes x 8-bit weights, every input code -128 and every weight code -128: the interior sum is
    9 * 16384 = 147456 and already the second tap's partial sum 32768 leaves a signed 16-bit lane."""
    c = _case(I8, 16, wbits=8, x_bits=8, bias=False, bn=False, fn=FN_NONE, act_bits=0, out_store=F32)
    N, H, W = c["map"]
    x = np.full((N, H, W, c["C"]), -128, np.int64)
    kernel = np.full((3, 3, c["C"], 1), -1.0, f32)
    return c, x, kernel
