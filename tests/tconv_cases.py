"""Cases and a numpy reference for the transposed convolution (include/qnn_abi_tconv.h).

The reference restates, in numpy float32 / int64 / float64, what the entry promises: the weight quantisers applied
elementwise to the Keras kernel (kh, kw, Cout, Cin), the scatter full[n, iy*s + ky, ix*s + kx, f] += x[n, iy, ix, c] *
w[ky, kx, f, c] cut or zero-extended to TensorFlow's output size, the float32 chain bias -> BN -> activation in the
reference's op order, and the encoding of the stores.  Kernel values and float inputs are multiples of 1/64, so every
summation order gives the same sum.  Nothing here imports the package under test; the quantisers, the chain and the
stores' encoding come from depthwise_cases.py.
"""
import itertools

import numpy as np

from depthwise_cases import (F32, BIN, T2, I4, I8, W_FLOAT, W_BINARY, W_QUANT, W_TERNARY, FN_NONE, FN_BINARY_TANH,  # noqa: F401
                             FN_QUANTIZED_TANH, FN_LEAKY_RELU, FN_QUANTIZED_RELU, FN_QUANTIZED_LEAKYRELU, QACTS, f32,
                             quantize_weights, chain, qact_code, words, encode, decode, signed_codes, random_codes,
                             values_of)

MAX_WINDOW, MAX_STRIDE = 8, 4


# ---- geometry (csrc/qnn_conv_geom.h, qnn_tconv_out_pad) ---------------------------------------------------------------------
def out_pad(size, k, s, same):
    """(out, pad_before) of one axis."""
    extra = max(k - s, 0)
    return (size * s, extra // 2) if same else (size * s + extra, 0)


def cut(full, s, same, H, W, kh, kw):
    """Rows [pt, pt + Ho) and columns [pl, pl + Wo) of the scatter `full` (N, (H-1)s+kh, (W-1)s+kw, F), zero beyond it."""
    Ho, pt = out_pad(H, kh, s, same)
    Wo, pl = out_pad(W, kw, s, same)
    out = np.zeros((full.shape[0], Ho, Wo, full.shape[3]), full.dtype)
    nr, nc = min(Ho, full.shape[1] - pt), min(Wo, full.shape[2] - pl)
    out[:, :nr, :nc] = full[:, pt:pt + nr, pl:pl + nc]
    return out


def tconv_sum(x, w, stride, same, dtype=np.int64):
    """The scatter of x (N, H, W, Cin) through w (kh, kw, Cout, Cin), no kernel flip, cut to the output size."""
    N, H, W, C = x.shape
    kh, kw, F, _ = w.shape
    s = stride
    full = np.zeros((N, (H - 1) * s + kh, (W - 1) * s + kw, F), dtype)
    xs, ws = x.astype(dtype), w.astype(dtype)
    for ky in range(kh):
        for kx in range(kw):
            full[:, ky:ky + (H - 1) * s + 1:s, kx:kx + (W - 1) * s + 1:s] += np.einsum("nhwc,fc->nhwf", xs, ws[ky, kx])
    return cut(full, s, same, H, W, kh, kw)


def int32_refused(kh, kw, s, cin, x_bits, wshift):
    """The entry's refusal: ceil(kh/s) * ceil(kw/s) * Cin * 2^(x_bits-1) * 2^wshift >= 2^31."""
    return -(-kh // s) * -(-kw // s) * cin * (1 << (x_bits - 1)) * (1 << wshift) >= (1 << 31)


def takes_mfma(c):
    """The host's route rule for the matrix-pipe form, restated (the tests' pointers are 16-byte aligned unless the case
    says misalign, and no test image reaches 2^31 bytes)."""
    kh, kw = c["window"]
    return (c["stride"] == 2 and kh == kw and 2 <= kh <= 4 and c["store"] in (I4, I8) and c["out_store"] == c["store"] and
            c["Cin"] % 64 == 0 and c["Cin"] <= 16384 and c["Cout"] % 16 == 0 and not c["misalign"])


def reference(case, x_codes_or_f32, kernel, bias, bn):
    """The expected output of one case: float32 values or integer codes, shaped (N, Ho, Wo, Cout)."""
    q, wcode, wshift = quantize_weights(kernel, case["wkind"], case.get("wbits", 0))
    if case["store"] == F32:
        v = tconv_sum(np.asarray(x_codes_or_f32, f32), q, case["stride"], case["same"], np.float64).astype(f32)
    else:
        acc = tconv_sum(signed_codes(x_codes_or_f32, case["store"]), wcode, case["stride"], case["same"])
        assert np.abs(acc).max(initial=0) < (1 << 24)          # the int32 -> float32 conversion is exact in every case
        xshift = case["x_bits"] - 1 if case["store"] in (I4, I8) else 0
        v = (acc.astype(f32) * f32(2.0 ** -(wshift + xshift))).astype(f32)
    return chain(v, bias, bn, case["fn"], case.get("act_bits", 0), case["out_store"])


# ---- the case table ------------------------------------------------------------------------------------------------------
WINDOWS = ((1, 1), (2, 2), (3, 3), (4, 4), (2, 3), (5, 5), (8, 8))
STRIDES = (1, 2, 3, 4)
MAPS = ((3, 1, 1), (3, 1, 5), (3, 3, 2), (3, 5, 4))        # N, H, W
CINS = (1, 3, 8, 9, 33)
COUTS = (1, 5, 8, 17)
STORES = (F32, BIN, T2, I4, I8)


def _case(store, Cin, Cout, **kw):
    c = dict(store=store, Cin=Cin, Cout=Cout, window=(3, 3), stride=2, same=True, map=MAPS[3], bias=True, bn=True,
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
    return "s%d_%dto%d_k%dx%d_s%d_%s_w%d.%d_x%d_fn%d.%d_o%d_%s%s%s_%s" % (
        c["store"], c["Cin"], c["Cout"], c["window"][0], c["window"][1], c["stride"], "same" if c["same"] else "valid",
        c["wkind"], c["wbits"], c["x_bits"], c["fn"], c["act_bits"], c["out_store"],
        "b" if c["bias"] else "", "n" if c["bn"] else "", "m" if c["misalign"] else "", "x".join(map(str, c["map"])))


def geometry_cases():
    """Every window x stride x padding on every store (k < s and k not a multiple of s included), the maps and channel
    counts walked round robin so that each appears with each store."""
    out = []
    combos = list(itertools.product(WINDOWS, STRIDES, (True, False)))
    for si, store in enumerate(STORES):
        for i, (window, stride, same) in enumerate(combos):
            j = i + si
            out.append(_case(store, CINS[j % 5], COUTS[(j // 2) % 4], window=window, stride=stride, same=same,
                             map=MAPS[(j // 3) % 4]))
    return out


def channel_cases():
    """Every Cin x Cout on every store (ragged last words, T2 pairs, one and several words per pixel) at 3x3 / 2 'same'
    and 2x2 / 2 'valid', maps alternating."""
    out = []
    for store in STORES:
        for i, (cin, cout) in enumerate(itertools.product(CINS, COUTS)):
            out.append(_case(store, cin, cout, window=(3, 3) if i % 2 else (2, 2), same=bool(i % 2), map=MAPS[i % 4]))
    return out


def weight_cases():
    """Each weight kind on each store whose rules allow it (qnn_tconv_prepack), x_bits at and below the store."""
    out = []
    for store, cin, cout in ((I4, 9, 5), (I8, 9, 5)):
        for wkind, wbits in ((W_BINARY, 1), (W_TERNARY, 1), (W_QUANT, 2), (W_QUANT, 4), (W_QUANT, 8)):
            if wkind == W_QUANT and wbits > store:
                continue
            for x_bits in sorted({2, 4, store}):
                out.append(_case(store, cin, cout, wkind=wkind, wbits=wbits, x_bits=x_bits))
    out.append(_case(T2, 33, 5, wkind=W_BINARY))
    for wkind, wbits in ((W_BINARY, 1), (W_TERNARY, 1), (W_QUANT, 2), (W_QUANT, 4), (W_QUANT, 8), (W_QUANT, 16)):
        out.append(_case(F32, 3, 5, wkind=wkind, wbits=wbits))
    return out


def epilogue_cases():
    """Each supported fn to each legal out_store, with bias and BN (negative scales among them) and without either."""
    out = []
    for store, cin, cout in ((I4, 9, 17), (I8, 8, 5), (BIN, 33, 8), (T2, 33, 17), (F32, 3, 5)):
        pairs = [(FN_NONE, 0, F32), (FN_LEAKY_RELU, 0, F32), (FN_BINARY_TANH, 0, F32), (FN_BINARY_TANH, 0, BIN),
                 (FN_BINARY_TANH, 0, I4), (FN_BINARY_TANH, 0, I8)]
        for fn in QACTS:
            pairs += [(fn, 4, F32), (fn, 2, I4), (fn, 4, I4), (fn, 4, I8), (fn, 6, I8), (fn, 8, I8)]
        for (fn, ab, os), (bias, bn) in itertools.product(pairs, ((True, True), (False, False))):
            out.append(_case(store, cin, cout, fn=fn, act_bits=ab, out_store=os, bias=bias, bn=bn, window=(3, 3), stride=2))
        out.append(_case(store, cin, cout, bias=True, bn=False))
        out.append(_case(store, cin, cout, bias=False, bn=True))
    return out


MFMA_MAPS = ((3, 1, 1), (3, 5, 1), (3, 1, 17), (3, 2, 15), (3, 5, 16), (3, 2, 33))


def mfma_cases():
    """I4 / I8 x windows 2, 3, 4 x both paddings on every map: ragged 16-pixel groups, single-row and single-column images
    (every neighbour tap outside), N = 3 (a wave's pixels never cross an image).  (Cin, Cout) alternates between (64, 16)
    and (128, 48) so that both meet every store, window and padding."""
    out = []
    i = 0
    for store, k, same in itertools.product((I4, I8), (2, 3, 4), (True, False)):
        for m in MFMA_MAPS:
            cin, cout = ((64, 16), (128, 48))[i % 2]
            i += 1
            out.append(_case(store, cin, cout, window=(k, k), stride=2, same=same, map=m))
        i += 1
    return out


def boundary_cases():
    """One shape just outside each edge of the route rule: they take the plain form."""
    base = dict(window=(3, 3), stride=2, same=True, map=(3, 2, 15))
    return [_case(I4, 32, 16, **base), _case(I4, 64, 8, **base), _case(I4, 64, 16, **dict(base, stride=1)),
            _case(I4, 64, 16, **dict(base, window=(5, 5))), _case(I8, 32, 16, **base), _case(I8, 64, 8, **base),
            _case(I4, 64, 16, **dict(base, window=(2, 3))), _case(I4, 64, 16, **dict(base, stride=3))]


# ---- maps on which a kernel's wave or item decode is not trivial ----------------------------------------------------------------
K_PG = 4                 # 16-pixel groups a wave of k_tc_mfma takes (csrc/qnn_tconv.hip)
MULTITASK_MAPS = (       # window, same, map
    (3, False, (2, 2, 21)), (3, True, (2, 4, 40)), (2, False, (2, 2, 21)), (4, False, (2, 2, 21)))


def phase_pixels(c):
    """Output pixels of one image per sub-pixel phase (row parity, column parity) of a stride-2 case, phase (0, 0) first."""
    _, H, W = c["map"]
    Ho = out_pad(H, c["window"][0], 2, c["same"])[0]
    Wo = out_pad(W, c["window"][1], 2, c["same"])[0]
    return [((Ho - rp + 1) // 2) * ((Wo - cp + 1) // 2) for rp in (0, 1) for cp in (0, 1)]


def wave_tasks(c):
    """(GT, waves) of k_tc_mfma's launch: GT wave tasks of K_PG groups per (image, phase, 32-filter block), sized by phase
    (0, 0), the largest; a task whose first group lies beyond its own phase returns at once."""
    GT = -(-(-(-phase_pixels(c)[0] // 16)) // K_PG)
    return GT, c["map"][0] * 4 * GT * (-(-c["Cout"] // 32))


def phase_groups(c, want):
    """Per image the 16-pixel groups of k_tc_mfma as arrays (pixels, Cout): each phase's pixels flattened row by row."""
    out = []
    for n in range(want.shape[0]):
        gs = []
        for rp in (0, 1):
            for cp in (0, 1):
                ph = want[n, rp::2, cp::2].reshape(-1, want.shape[-1])
                gs += [ph[i:i + 16] for i in range(0, len(ph), 16)]
        out.append(gs)
    return out


def multitask_cases():
    """Maps on which k_tc_mfma's wave decode (image, phase, K_PG groups from g0, filter block) and the plain form's (pixel,
    word group) are not trivial.  Every case carries the `seed` of its inputs.
    matrix pipe, I4 and I8, (Cin, Cout) = (64, 16) (a half-filled filter block) and (128, 48) (two blocks):
      k = 3 'valid' (2, 2, 21)  phases of 66 / 63 / 44 / 42 pixels, GT = 2: three phases return early at g0 == 4
      k = 3 'same'  (2, 4, 40)  160 pixels per phase, GT = 3
      k = 2 'valid' (2, 2, 21)  42 per phase, GT = 1   } equal phases
      k = 4 'valid' (2, 2, 21)  66 per phase, GT = 2   }
      k = 3 'same'  (70, 1, 1)  I4 only: one pixel per phase, the image index runs to 69 over 70 workgroups
    plain form, I8 16 -> 16 at 3x3 / 2 'same' on (2, 5, 9): 360 items at V = 4, and off alignment 1440 at V = 1."""
    out = []
    for store in (I4, I8):
        for cin, cout in ((64, 16), (128, 48)):
            for k, same, m in MULTITASK_MAPS:
                out.append(_case(store, cin, cout, window=(k, k), same=same, map=m, seed=0))
    out.append(_case(I4, 64, 16, map=(70, 1, 1), seed=0))
    for misalign in (False, True):
        out.append(_case(I8, 16, 16, map=(2, 5, 9), misalign=misalign, seed=0))
    return out


def make_inputs(c, seed=0):
    """Deterministic inputs of a case: (x codes or float32 values, kernel (kh, kw, Cout, Cin), bias or None, (inv, shift)
    or None).  Kernel values and float inputs are multiples of 1/64 in [-1, 1]; bias and BN constants are small dyadic
    numbers (BN scales of both signs), so pre-activations land on rounding ties and clip edges.  Every image of a batch
    has its own values."""
    rs = np.random.RandomState(2000 + seed)
    N, H, W = c["map"]
    kh, kw = c["window"]
    if c["store"] == F32:
        x = (rs.randint(-64, 65, (N, H, W, c["Cin"])) / 64.0).astype(f32)
    else:
        x = random_codes(rs, (N, H, W, c["Cin"]), c["store"], c["x_bits"])
    kernel = (rs.randint(-64, 65, (kh, kw, c["Cout"], c["Cin"])) / 64.0).astype(f32)
    bias = (rs.randint(-8, 9, c["Cout"]) / 16.0).astype(f32) if c["bias"] else None
    bn = None
    if c["bn"]:
        # wide sums (many channels) are brought back into the clip's range by a smaller scale
        lo = -2 - int(np.log2(max(c["Cin"], 1))) // 2
        bn = ((2.0 ** rs.randint(lo, lo + 4, c["Cout"])).astype(f32) * rs.choice([-1, 1], c["Cout"]).astype(f32),
              (rs.randint(-8, 9, c["Cout"]) / 32.0).astype(f32))
    return x, kernel, bias, bn


# ---- the output-size rule, written out by hand for an axis of 5 cells: (k, s) -> (valid out, same pad_before); the
# 'same' output is 5 * s and the 'valid' pad_before is 0 ------------------------------------------------------------------------
SIZE_TABLE_IN = 5
SIZE_TABLE = {
    (1, 1): (5, 0), (2, 1): (6, 0), (3, 1): (7, 1), (4, 1): (8, 1), (5, 1): (9, 2), (8, 1): (12, 3),
    (1, 2): (10, 0), (2, 2): (10, 0), (3, 2): (11, 0), (4, 2): (12, 1), (5, 2): (13, 1), (8, 2): (16, 3),
    (1, 3): (15, 0), (2, 3): (15, 0), (3, 3): (15, 0), (4, 3): (16, 0), (5, 3): (17, 1), (8, 3): (20, 2),
    (1, 4): (20, 0), (2, 4): (20, 0), (3, 4): (20, 0), (4, 4): (20, 0), (5, 4): (21, 0), (8, 4): (24, 2),
}
