"""Cases and a numpy reference for the grouped convolution (include/qnn_abi_gconv.h).

The reference restates, in numpy float32 / int64 / float64, what the entry promises: the weight quantisers applied
elementwise to the Keras kernel (kh, kw, Cin / g, Cout) -- the ternary cutoff over this whole kernel --, filter f of group
f // Fg summed over the in-bounds taps and its group's Cg input channels, the float32 chain bias -> BN -> activation in
the reference's op order, and the encoding of the stores.  Kernel values and float inputs are multiples of 1/64, so every
summation order gives the same sum.  The route rule and the slot plan of csrc/qnn_gconv_plan.h are restated here too.
Nothing here imports the package under test; the quantisers, the chain and the stores' encoding come from
depthwise_cases.py.
"""
import itertools

import numpy as np

from depthwise_cases import (F32, BIN, T2, I4, I8, W_FLOAT, W_BINARY, W_QUANT, W_TERNARY, FN_NONE, FN_BINARY_TANH,  # noqa: F401
                             FN_QUANTIZED_TANH, FN_LEAKY_RELU, FN_QUANTIZED_RELU, FN_QUANTIZED_LEAKYRELU, QACTS, f32,
                             out_pad, quantize_weights, chain, qact_code, words, encode, decode, signed_codes,
                             random_codes, values_of)

MAX_WINDOW = 7
MAX_RUN = 16384


# ---- the convolution -------------------------------------------------------------------------------------------------------
def gconv_sum(x, w, groups, stride, same, dil=(1, 1), dtype=np.int64):
    """sum over the in-bounds taps and the group's channels of x[n, y, x, grp * Cg + c] * w[ky, kx, c, f], grp = f // Fg
    -> (N, Ho, Wo, Cout), accumulated in `dtype` in (ky, kx, c) order (exact for the tests' values in any order)."""
    N, H, W, Cin = x.shape
    kh, kw, Cg, Cout = w.shape
    assert Cin == Cg * groups and Cout % groups == 0
    Fg = Cout // groups
    Ho, pt = out_pad(H, kh, stride, same, dil[0])
    Wo, pl = out_pad(W, kw, stride, same, dil[1])
    acc = np.zeros((N, Ho, Wo, Cout), dtype)
    xs = x.astype(dtype).reshape(N, H, W, groups, Cg)
    ws = w.astype(dtype).reshape(kh, kw, Cg, groups, Fg)
    for ky in range(kh):
        for kx in range(kw):
            for oy in range(Ho):
                yy = oy * stride - pt + ky * dil[0]
                if not 0 <= yy < H:
                    continue
                for ox in range(Wo):
                    xx = ox * stride - pl + kx * dil[1]
                    if 0 <= xx < W:
                        acc[:, oy, ox] += np.einsum("ngc,cgf->ngf", xs[:, yy, xx], ws[ky, kx]).reshape(N, Cout)
    return acc


def expand_block_diagonal(kernel, groups):
    """Keras grouped kernel (kh, kw, Cg, Cout) -> the full HWIO kernel (kh, kw, Cin, Cout), zero off the diagonal blocks."""
    kh, kw, Cg, Cout = kernel.shape
    Fg = Cout // groups
    full = np.zeros((kh, kw, Cg * groups, Cout), kernel.dtype)
    for g in range(groups):
        full[:, :, g * Cg:(g + 1) * Cg, g * Fg:(g + 1) * Fg] = kernel[:, :, :, g * Fg:(g + 1) * Fg]
    return full


def int32_refused(kh, kw, Cg, x_bits, wshift):
    """The entry's refusal: kh * kw * Cg * 2^(x_bits-1) * 2^wshift >= 2^31."""
    return kh * kw * Cg * (1 << (x_bits - 1)) * (1 << wshift) >= (1 << 31)


# ---- the tile plan and the route rule, restated (csrc/qnn_gconv_plan.h) ----------------------------------------------------
def plan(kh, kw, cin, cout, groups):
    """None where the shape is not eligible, else dict(t, R, spt, slots, steps, tiles)."""
    Cg, Fg = cin // groups, cout // groups
    if cout % 16 or (Fg % 16 and 16 % Fg):
        return None
    t = 1 if Fg % 16 == 0 else 16 // Fg
    R = t * Cg
    if R % 16 or R > MAX_RUN:
        return None
    spt = R // 16
    slots = kh * kw * spt
    steps = -(-slots // 4)
    if (cout // 16) * steps * 1024 >= 1 << 31:
        return None
    return dict(Cg=Cg, Fg=Fg, t=t, R=R, spt=spt, slots=slots, steps=steps, tiles=cout // 16)


def tile_channel(p, tile):
    return (16 * tile // p["Fg"]) * p["Cg"] if p["t"] == 1 else tile * p["R"]


def slot(p, s):
    """(tap, chunk) of slot s, None for a padding slot."""
    return divmod(s, p["spt"]) if 0 <= s < p["slots"] else None


def takes_mfma(c):
    """The host's route rule for the matrix-pipe form (the tests' pointers are 16-byte aligned unless the case says
    misalign, and no test image reaches 2^31 bytes)."""
    kh, kw = c["window"]
    return (c["store"] in (I4, I8) and c["out_store"] == c["store"] and not c["misalign"] and
            plan(kh, kw, c["Cin"], c["Cout"], c["groups"]) is not None)


def reference(case, x_codes_or_f32, kernel, bias, bn):
    """The expected output of one case: float32 values or integer codes, shaped (N, Ho, Wo, Cout)."""
    q, wcode, wshift = quantize_weights(kernel, case["wkind"], case.get("wbits", 0))
    if case["store"] == F32:
        v = gconv_sum(np.asarray(x_codes_or_f32, f32), q, case["groups"], case["stride"], case["same"], case["dil"],
                      np.float64).astype(f32)
    else:
        acc = gconv_sum(signed_codes(x_codes_or_f32, case["store"]), wcode, case["groups"], case["stride"], case["same"],
                        case["dil"])
        assert np.abs(acc).max(initial=0) < (1 << 31)
        xshift = case["x_bits"] - 1 if case["store"] in (I4, I8) else 0
        v = (acc.astype(np.int32).astype(f32) * f32(2.0 ** -(wshift + xshift))).astype(f32)
    return chain(v, bias, bn, case["fn"], case.get("act_bits", 0), case["out_store"])


# ---- the case table ------------------------------------------------------------------------------------------------------
MAP = (2, 5, 7)            # N, H, W
STORES = (F32, BIN, T2, I4, I8)


def _case(store, Cg, Fg, groups, **kw):
    c = dict(store=store, Cg=Cg, Fg=Fg, groups=groups, Cin=Cg * groups, Cout=Fg * groups, window=(3, 3), stride=1,
             same=True, dil=(1, 1), map=MAP, bias=True, bn=True, misalign=False, extreme=False)
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
    return "s%d_g%d_%dx%d_k%dx%d_s%d_d%dx%d_%s_w%d.%d_x%d_fn%d.%d_o%d_%s%s%s%s_%s" % (
        c["store"], c["groups"], c["Cg"], c["Fg"], c["window"][0], c["window"][1], c["stride"], c["dil"][0], c["dil"][1],
        "same" if c["same"] else "valid", c["wkind"], c["wbits"], c["x_bits"], c["fn"], c["act_bits"], c["out_store"],
        "b" if c["bias"] else "", "n" if c["bn"] else "", "m" if c["misalign"] else "", "e" if c["extreme"] else "",
        "x".join(map(str, c["map"])))


# (Cg, Fg) whose group edges fall inside input words and whose output words straddle groups
GROUP_SHAPES = {I4: ((3, 1), (3, 3), (5, 5), (8, 3)), I8: ((3, 5), (1, 1), (5, 3)), BIN: ((5, 1), (5, 3), (33, 5)),
                T2: ((3, 3), (33, 5), (5, 1)), F32: ((3, 1), (2, 5))}
GEOMETRIES = (  # window, stride, same, dil, map
    ((1, 1), 1, True, (1, 1), MAP), ((3, 3), 1, True, (1, 1), MAP), ((5, 5), 1, True, (1, 1), MAP),
    ((1, 7), 1, True, (1, 1), MAP), ((7, 1), 1, False, (1, 1), (2, 9, 3)), ((3, 3), 2, True, (1, 1), MAP),
    ((3, 3), 2, False, (1, 1), MAP), ((3, 3), 1, True, (2, 2), MAP), ((3, 3), 1, False, (1, 3), (2, 5, 9)),
    ((3, 3), 1, True, (1, 1), (3, 1, 1)), ((3, 3), 1, True, (1, 1), (1, 1, 17)), ((5, 5), 2, True, (1, 1), (2, 2, 2)),
)


def plain_cases():
    """Every store with g in {1, 2, 3, 4} on the group shapes above, the geometries walked round robin."""
    out, i = [], 0
    for store in STORES:
        for (Cg, Fg), g in itertools.product(GROUP_SHAPES[store], (1, 2, 3, 4)):
            for k in range(3):
                window, stride, same, dil, m = GEOMETRIES[(i + k * 4) % len(GEOMETRIES)]
                out.append(_case(store, Cg, Fg, g, window=window, stride=stride, same=same, dil=dil, map=m))
            i += 1
    return out


def weight_cases():
    """Each weight kind on each store whose rules allow it, x_bits at and below the store."""
    out = []
    for store, Cg, Fg, g in ((I4, 3, 3, 3), (I8, 3, 5, 2)):
        for wkind, wbits in ((W_BINARY, 1), (W_TERNARY, 1), (W_QUANT, 2), (W_QUANT, 4), (W_QUANT, 8)):
            if wkind == W_QUANT and wbits > store:
                continue
            for x_bits in sorted({2, 4, store}):
                out.append(_case(store, Cg, Fg, g, wkind=wkind, wbits=wbits, x_bits=x_bits))
    out.append(_case(T2, 33, 5, 2, wkind=W_BINARY))
    for wkind, wbits in ((W_BINARY, 1), (W_TERNARY, 1), (W_QUANT, 2), (W_QUANT, 4), (W_QUANT, 8), (W_QUANT, 16)):
        out.append(_case(F32, 3, 5, 2, wkind=wkind, wbits=wbits))
    return out


def _fn_pairs():
    pairs = [(FN_NONE, 0, F32), (FN_LEAKY_RELU, 0, F32), (FN_BINARY_TANH, 0, F32), (FN_BINARY_TANH, 0, BIN),
             (FN_BINARY_TANH, 0, I4), (FN_BINARY_TANH, 0, I8)]
    for fn in QACTS:
        pairs += [(fn, 4, F32), (fn, 2, I4), (fn, 4, I4), (fn, 4, I8), (fn, 8, I8)]
    return pairs


def epilogue_cases():
    """Each supported fn to each legal out_store, with bias and BN (negative scales among them) and without either."""
    out = []
    for store, Cg, Fg, g in ((I4, 3, 3, 3), (I8, 3, 5, 2), (BIN, 5, 3, 3), (T2, 33, 5, 2), (F32, 3, 1, 4)):
        for (fn, ab, os), (bias, bn) in itertools.product(_fn_pairs(), ((True, True), (False, False))):
            out.append(_case(store, Cg, Fg, g, fn=fn, act_bits=ab, out_store=os, bias=bias, bn=bn))
    return out


MFMA_SHAPES = ((4, 4, 4), (4, 4, 8), (8, 8, 4), (16, 16, 2), (16, 32, 2), (32, 16, 2), (48, 16, 2), (64, 16, 2), (128, 16, 2),
               (8, 2, 8), (1, 1, 16), (2, 1, 16))      # (Cg, Fg, g)
MFMA_GEOMS = (  # window, stride, same, dil, map
    ((1, 1), 1, True, (1, 1), (3, 5, 5)), ((2, 2), 1, True, (1, 1), (3, 1, 17)), ((3, 3), 1, True, (1, 1), (3, 5, 5)),
    ((5, 5), 1, True, (1, 1), (3, 17, 3)), ((1, 7), 1, True, (1, 1), (3, 1, 17)), ((3, 3), 1, True, (2, 2), (3, 5, 5)),
    ((3, 3), 2, True, (1, 1), (3, 17, 3)), ((3, 3), 2, False, (1, 1), (3, 5, 5)), ((3, 3), 1, True, (1, 1), (3, 1, 1)),
)


def mfma_cases():
    """I4 and I8 on every (Cg, Fg, g) of the list; each shape meets three geometries, round robin, so that every geometry
    meets both stores."""
    out, i = [], 0
    for store in (I4, I8):
        for Cg, Fg, g in MFMA_SHAPES:
            for k in range(3):
                window, stride, same, dil, m = MFMA_GEOMS[(i + 3 * k) % len(MFMA_GEOMS)]
                out.append(_case(store, Cg, Fg, g, window=window, stride=stride, same=same, dil=dil, map=m))
            i += 1
    return out


def boundary_cases():
    """One shape just outside each shape edge of the route rule: R = 12, Fg = 24, Cout = 8."""
    return [_case(I4, 3, 4, 4), _case(I8, 3, 4, 4), _case(I4, 16, 24, 2), _case(I8, 16, 24, 2), _case(I4, 16, 8, 1),
            _case(I8, 32, 4, 2)]


# ---- maps on which a kernel's wave or item decode is not trivial ----------------------------------------------------------------
K_PG = 4                 # 16-pixel groups a wave of k_gc_mfma takes (csrc/qnn_gconv.hip)
MULTITASK_GEOMS = (      # stride, same, map: all 3x3
    (1, True, (2, 9, 9)), (1, True, (2, 5, 29)), (2, False, (3, 17, 9)), (2, True, (2, 19, 15)))
MULTITASK_SHAPES = ((4, 4, 4), (16, 32, 2), (2, 1, 16))        # one tile of 4 groups, 4 tiles, one tile of 16 groups


def wave_tasks(c):
    """(output pixels of an image, its 16-pixel groups, GT, waves) of k_gc_mfma's launch: GT wave tasks of K_PG groups per
    (image, 16-filter tile), the tile fastest."""
    N, H, W = c["map"]
    npix = out_pad(H, c["window"][0], c["stride"], c["same"], c["dil"][0])[0] * \
        out_pad(W, c["window"][1], c["stride"], c["same"], c["dil"][1])[0]
    groups = -(-npix // 16)
    GT = -(-groups // K_PG)
    return npix, groups, GT, N * GT * (c["Cout"] // 16)


def multitask_cases():
    """Maps on which k_gc_mfma's wave decode (image, K_PG groups from g0, tile) and the plain form's (pixel, word group) are
    not trivial.  Every case carries the `seed` of its inputs.
    matrix pipe, I4 and I8, every shape of MULTITASK_SHAPES at 3x3:
      'same'  / 1 (2, 9, 9)    81 pixels = 6 groups, GT = 2: the second task holds a full group, a one-pixel group and two
                               groups beyond the image
      'same'  / 1 (2, 5, 29)   145 pixels = 10 groups, GT = 3: the third task's pair is a full group and a one-pixel group,
                               so 15 lanes of an int4 pair have one valid member; with one tile 6 waves: the second workgroup
                               is half filled
      'valid' / 2 (3, 17, 9)   8 x 4 = 32 pixels, GT = 1: the control
      'same'  / 2 (2, 19, 15)  10 x 8 = 80 pixels = 5 groups, GT = 2: the second task is group 4 alone, its int4 pair
                               partner beyond the image
      'same'  / 1 (70, 1, 1)   I4 (4, 4, 4) only: one pixel per image, 70 waves, the image index runs to 69
    plain form, I4 (Cg 8, Fg 8, g 4) to float32 (the route rule wants out_store == store) on (2, 9, 11): 1584 items at V = 4,
    and off alignment 6336 at V = 1."""
    out = []
    for store in (I4, I8):
        for Cg, Fg, g in MULTITASK_SHAPES:
            for stride, same, m in MULTITASK_GEOMS:
                # seed 0 leaves 0.518 of this case's codes at the clip ends (test_gconv_cpu.py caps that at a half), seed 5 0.351
                seed = 5 if (store, Cg, m) == (I4, 2, (3, 17, 9)) else 0
                out.append(_case(store, Cg, Fg, g, stride=stride, same=same, map=m, seed=seed))
    out.append(_case(I4, 4, 4, 4, map=(70, 1, 1), seed=0))
    for misalign in (False, True):
        out.append(_case(I4, 8, 8, 4, map=(2, 9, 11), out_store=F32, misalign=misalign, seed=0))
    return out


# the route rule on its boundary table: (kh, kw, Cin, Cout, groups) -> eligible
ROUTE_TABLE = (
    ((3, 3, 16, 16, 4), True), ((3, 3, 12, 16, 4), False), ((3, 3, 32, 48, 2), False), ((3, 3, 32, 8, 2), False),
    ((3, 3, 16, 16, 16), True), ((3, 3, 32, 16, 16), True), ((3, 3, 16, 32, 16), False), ((1, 1, 64, 64, 1), True),
    ((7, 7, 16384, 16, 1), True), ((7, 7, 16400, 16, 1), False), ((3, 3, 2048, 32, 2), True), ((3, 3, 1024, 1024, 32), True),
    ((3, 3, 64, 16, 8), True), ((3, 3, 64, 24, 8), False), ((3, 3, 32, 64, 2), True), ((3, 3, 24, 64, 2), False),
)


def make_inputs(c, seed=0):
    """Deterministic inputs of a case: (x codes or float32 values, kernel (kh, kw, Cg, Cout), bias or None, (inv, shift)
    or None).  Kernel values and float inputs are multiples of 1/64 in [-1, 1]; bias and BN constants are small dyadic
    numbers (BN scales of both signs).  Packed inputs carry the extreme codes; `extreme` sets every input and weight to the
    most negative code."""
    rs = np.random.RandomState(3000 + seed)
    N, H, W = c["map"]
    kh, kw = c["window"]
    if c["store"] == F32:
        x = (rs.randint(-64, 65, (N, H, W, c["Cin"])) / 64.0).astype(f32)
    else:
        x = random_codes(rs, (N, H, W, c["Cin"]), c["store"], c["x_bits"])
        if c["store"] in (I4, I8):
            lo, hi = -(1 << (c["x_bits"] - 1)), (1 << (c["x_bits"] - 1)) - 1
            x.reshape(-1)[::7] = lo
            x.reshape(-1)[3::11] = hi
            if c["extreme"]:
                x[...] = lo
    kernel = (rs.randint(-64, 65, (kh, kw, c["Cg"], c["Cout"])) / 64.0).astype(f32)
    if c["extreme"]:
        kernel[...] = -1.0
    bias = (rs.randint(-8, 9, c["Cout"]) / 16.0).astype(f32) if c["bias"] else None
    bn = None
    if c["bn"]:
        lo = -2 - int(np.log2(max(c["Cg"] * kh * kw // 9, 1))) // 2
        bn = ((2.0 ** rs.randint(lo, lo + 4, c["Cout"])).astype(f32) * rs.choice([-1, 1], c["Cout"]).astype(f32),
              (rs.randint(-8, 9, c["Cout"]) / 32.0).astype(f32))
    return x, kernel, bias, bn
