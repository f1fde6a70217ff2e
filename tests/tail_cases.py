"""Case tables and independent references for everything behind the convolutions: the dense entry (qnn_dense_forward), the
packed average pool, the softmax, pack / unpack and the elementwise activations.  A plain module (no tests in it): the CPU
test (test_tail_cases_cpu.py) proves the tables build, cover every branch of the dispatch and agree with the oracle; the GPU
test (test_gpu_tail.py) compares the HIP kernels with the references below.

The references are written out in numpy on integer codes (int64) or in float64; the oracle (oracle/qnn_oracle.py) is used
only for the quantizers and for the float32 operations of the epilogue, never for a contraction."""
import os
import re

import numpy as np

from oracle import qnn_oracle as O

F32 = np.float32
STORE_F32, STORE_BIN, STORE_T2, STORE_I4, STORE_I8 = 0, 1, 2, 4, 8          # include/qnn_abi.h
PACKED = (STORE_BIN, STORE_I4, STORE_I8, STORE_T2)
STORE_NAME = {STORE_F32: "f32", STORE_BIN: "bin", STORE_T2: "t2", STORE_I4: "i4", STORE_I8: "i8"}
PACKED_FILL = 0x5a5a5a5a            # what the GPU tests pre-fill packed outputs with; no reference may contain it
K_BLOCK = 256                       # threads per block of the dense kernels (kBlock, csrc/qnn_conv.hip)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "quantizedneuralnetworks-keras-tensorflow_amd", "csrc")


# ---------------------------------------------------------------------------------------------------------------------
# packed storage, from the layout rules of include/qnn_abi.h
# ---------------------------------------------------------------------------------------------------------------------
def per_word(store):
    return {STORE_BIN: 32, STORE_T2: 32, STORE_I4: 8, STORE_I8: 4}[store]


def words(store, channels):
    """qnn_words: packed words per pixel (T2: a mask and a sign word per 32 channels)."""
    n = -(-channels // per_word(store))
    return 2 * n if store == STORE_T2 else n


def pack_words(codes, store):
    """Integer codes (pixels, C) -> uint32 words (pixels, words(store, C)).  Channel c of a pixel sits in word c // per_word,
    field c % per_word (fields from the least significant bit up), as a two's-complement code of the field's width; BIN: bit
    = 1 <=> +1; T2: a mask word (code != 0) followed by a sign word (code > 0) per 32 channels; pad fields are zero."""
    codes = np.asarray(codes)
    P, C = codes.shape
    pw = per_word(store)
    cw = -(-C // pw)
    bits = 32 // pw

    def fold(fields):                       # (P, C) non-negative field values -> (P, cw) words
        f = np.zeros((P, cw * pw), dtype=np.uint32)
        f[:, :C] = fields
        f = f.reshape(P, cw, pw)
        f <<= (np.arange(pw, dtype=np.uint32) * np.uint32(bits))
        return np.bitwise_or.reduce(f, axis=-1)

    if store == STORE_BIN:
        return fold(codes > 0)
    if store == STORE_T2:
        out = np.empty((P, cw, 2), dtype=np.uint32)
        out[:, :, 0] = fold(codes != 0)
        out[:, :, 1] = fold(codes > 0)
        return out.reshape(P, 2 * cw)
    return fold(codes.astype(np.int64) & ((1 << bits) - 1))


def code_range(store, bits):
    """(lowest, highest) code of `bits`-bit activations in `store`."""
    if store in (STORE_BIN, STORE_T2) or bits == 1:
        return -1, 1
    return -(1 << (bits - 1)), (1 << (bits - 1)) - 1


def random_codes(rng, shape, store, bits):
    """Random activation codes: BIN and 1-bit codes are +-1, T2 {-1, 0, +1}, otherwise the whole two's-complement range."""
    if store == STORE_T2:
        return rng.integers(-1, 2, shape).astype(np.int8)
    if store == STORE_BIN or bits == 1:
        return (rng.integers(0, 2, shape) * 2 - 1).astype(np.int8)
    lo, hi = code_range(store, bits)
    return rng.integers(lo, hi + 1, shape).astype(np.int8)


def code_scale(store, bits):
    """value = code * code_scale."""
    return 1.0 if store in (STORE_BIN, STORE_T2) else 2.0 ** -(bits - 1)


# ---------------------------------------------------------------------------------------------------------------------
# dense
# ---------------------------------------------------------------------------------------------------------------------
def dense_ipb(units):
    """(kernel form, images per block) launch_dense picks for `units` when kwords % 16 == 0 / otherwise."""
    if units <= 16:
        return ("split", K_BLOCK // (16 * 4)), ("up16", K_BLOCK // 16)
    if units <= 64:
        return (("up64", K_BLOCK // 64),) * 2
    if units <= 256:
        return (("up256", K_BLOCK // 256),) * 2
    return ((None, 0),) * 2


def dense_branch(c):
    """The branch of route_dense / launch_dense a case takes, from the predicates the dispatch uses.  `kwords` is
    qnn_words(store, K) (a dense layer has one tap)."""
    if c["res"]:
        return "residual"                                   # route_dense has no CAP_RES
    if c["out_store"] != STORE_F32:
        return "packed_out"                                 # route_dense declines
    if c["x_store"] == STORE_F32:
        return "f32_vec4" if c["K"] % 4 == 0 else "f32_scalar"      # k_dense_f32in: (cin & 3) == 0
    kwords = words(c["x_store"], c["K"])
    if kwords % 4 != 0:
        return "kwords_not_4"                               # route_dense declines
    if c["units"] <= 16 and kwords % 16 == 0:
        return "split"
    if c["units"] <= 16:
        return "up16"
    if c["units"] <= 64:
        return "up64"
    if c["units"] <= 256:
        return "up256"
    return "units_over_256"                                 # launch_dense declines


def dense_family(c):
    """"dense" if one of the dense kernels computes the case, "conv" if it lands on a convolution route at H = W = 1."""
    return "dense" if dense_branch(c) in ("f32_vec4", "f32_scalar", "split", "up16", "up64", "up256") else "conv"


def _k_for(store, kwords, short=0):
    """The K whose packed row has `kwords` words with `short` fields of the last word unused (derived from words())."""
    K = (kwords // 2 if store == STORE_T2 else kwords) * per_word(store) - short
    assert words(store, K) == kwords, (store, kwords, short)
    return K


def _case(x_store, x_bits, wkind, wbits, N, K, units, bias=True, bn=None, fn="none", act_bits=0, out_store=STORE_F32,
          res=False, fill=None, seed=0, why="", boundary=False, xkind="grid"):
    """bn: None, "pos" or "neg" (every gamma negative).  fill: None, "max" (all codes at the top), "min" (at the bottom),
    "alternating" (top, bottom, top, ... along K in both operands), "min_max" (activations at the bottom, weights at the
    top).  xkind (float32 input only): "grid" (codes / 2^(x_bits-1)), "normal", "cancel".  boundary: the row is there for a
    route boundary and the GPU test asserts its kernel family."""
    return dict(x_store=x_store, x_bits=x_bits, wkind=wkind, wbits=wbits, N=N, K=K, units=units, bias=bias, bn=bn, fn=fn,
                act_bits=act_bits, out_store=out_store, res=res, fill=fill, seed=seed, why=why, boundary=boundary, xkind=xkind)


# the operand pair each packed storage is exercised with on the boundary rows: (x_bits, wkind, wbits)
_PAIR = {STORE_BIN: (1, "binary", 1), STORE_T2: (1, "ternary", 1), STORE_I4: (4, "quantized", 4), STORE_I8: (8, "quantized", 8)}
# K that does not fill the last packed word, two per storage
PARTIAL_K = {STORE_BIN: (100, 1000), STORE_I4: (20, 1001), STORE_I8: (6, 1022), STORE_T2: (33, 1000)}
BOUNDARY_UNITS = (1, 10, 16, 17, 64, 65, 256, 257, 1000)
F32_CIN = (1, 3, 4, 63, 64, 255, 256, 257, 512, 4097)
F32_UNITS = (1, 10, 1000)


def _dense_table():
    t = []
    for s in PACKED:
        xb, wk, wb = _PAIR[s]
        # ---- every route boundary of launch_dense: units x kwords class.  kwords = 32 (% 16 == 0), 12 (% 4 == 0, not 16),
        #      6 (% 4 != 0: route_dense declines, a conv route at H = W = 1 takes the call)
        for units in BOUNDARY_UNITS:
            for kwords, kw_why in ((32, "kwords % 16 == 0"), (12, "kwords % 4 == 0, % 16 != 0"), (6, "kwords % 4 != 0")):
                t.append(_case(s, xb, wk, wb, 5, _k_for(s, kwords), units, boundary=True,
                               why="units %d, %s" % (units, kw_why)))
        # ---- K that does not fill the last packed word (pad fields must not count; BIN: cin - 2 * popcount)
        for K in PARTIAL_K[s]:
            for units in (10, 65):
                t.append(_case(s, xb, wk, wb, 6, K, units, boundary=True, why="K = %d leaves pad fields in the last word" % K))
        # one more per storage that is sure to reach a dense kernel with pad fields in the last word (kwords = 16 and 4)
        for kwords, units in ((16, 10), (4, 10), (4, 40), (4, 200)):
            t.append(_case(s, xb, wk, wb, 6, _k_for(s, kwords, short=3), units, boundary=True,
                           why="kwords = %d with 3 pad fields" % kwords))
        # ---- N against the images per block of each kernel form (ipb = 4, 16, 4, 1)
        for form, units, kwords in (("split", 10, 16), ("up16", 10, 12), ("up64", 40, 8), ("up256", 200, 8)):
            ipb = dict(dense_ipb(units))[form]
            for N in sorted({0, 1, ipb - 1, ipb, ipb + 1}):
                t.append(_case(s, xb, wk, wb, N, _k_for(s, kwords), units, boundary=N > 0,
                               why="N = %d against %d images per block of %s" % (N, ipb, form)))
    # the heads of the headline network (1024 -> 10 at N = 4096) and of the ImageNet ResNet (512 -> 1000 at N = 64)
    t.append(_case(STORE_I4, 4, "quantized", 4, 4096, 1024, 10, bn="pos", boundary=True, why="headline head, N = 4096"))
    t.append(_case(STORE_BIN, 1, "binary", 1, 4096, 1024, 10, bn="pos", boundary=True, why="full-bnn head, N = 4096"))
    t.append(_case(STORE_I4, 4, "quantized", 4, 64, 512, 1000, why="ImageNet head 512 -> 1000, N = 64"))
    t.append(_case(STORE_I8, 8, "quantized", 8, 64, 512, 1000, why="ImageNet head 512 -> 1000, N = 64, 8 bit"))
    # ---- widths: activations 1..4 bit in I4 storage, 5 and 8 (and narrower) in I8 storage; every weight kind
    for xb in (1, 2, 3, 4):
        for wk, wb in (("binary", 1), ("ternary", 1), ("quantized", 2), ("quantized", 3), ("quantized", 4)):
            t.append(_case(STORE_I4, xb, wk, wb, 7, 256, 10, why="I4: %d-bit activations, %s %d weights (split)" % (xb, wk, wb)))
            t.append(_case(STORE_I4, xb, wk, wb, 7, 96, 33, why="I4: %d-bit activations, %s %d weights (up64)" % (xb, wk, wb)))
    for xb in (1, 3, 5, 8):
        for wk, wb in (("binary", 1), ("ternary", 1), ("quantized", 2), ("quantized", 5), ("quantized", 8)):
            t.append(_case(STORE_I8, xb, wk, wb, 7, 128, 10, why="I8: %d-bit activations, %s %d weights (split)" % (xb, wk, wb)))
            t.append(_case(STORE_I8, xb, wk, wb, 7, 48, 100, why="I8: %d-bit activations, %s %d weights (up256)" % (xb, wk, wb)))
    t.append(_case(STORE_T2, 1, "binary", 1, 7, 512, 10, why="T2: ternary activations, binary weights with a full mask"))
    t.append(_case(STORE_T2, 1, "binary", 1, 7, 100, 40, why="T2: binary weights, pad fields"))
    # ---- epilogues on every storage: bias / BN sign / activation, the residual merge, packed outputs
    for s in PACKED:
        xb, wk, wb = _PAIR[s]
        for units, kwords in ((10, 16), (40, 8)):
            K = _k_for(s, kwords, short=1)
            t.append(_case(s, xb, wk, wb, 9, K, units, bias=False, why="no bias, no BN"))
            t.append(_case(s, xb, wk, wb, 9, K, units, bias=False, bn="neg", why="BN with negative gamma, no bias"))
            t.append(_case(s, xb, wk, wb, 9, K, units, bn="neg", fn="binary_tanh", why="bias, BN (gamma < 0), binary_tanh"))
            t.append(_case(s, xb, wk, wb, 9, K, units, bn="pos", fn="binary_tanh", why="bias, BN, binary_tanh"))
            for nb in (2, 4, 8):
                t.append(_case(s, xb, wk, wb, 9, K, units, bn="pos", fn="quantized_tanh", act_bits=nb,
                               why="bias, BN, quantized_tanh %d" % nb))
            t.append(_case(s, xb, wk, wb, 9, K, units, bn="neg", res=True, why="float32 residual, post_scale 0.5"))
            t.append(_case(s, xb, wk, wb, 9, K, units, bn="pos", res=True, fn="quantized_tanh", act_bits=4,
                           why="float32 residual, post_scale 0.5, quantized_tanh 4"))
            t.append(_case(s, xb, wk, wb, 9, K, units, bn="pos", fn="binary_tanh", out_store=STORE_BIN,
                           why="packed BIN output: route_dense declines"))
            t.append(_case(s, xb, wk, wb, 9, K, units, bn="neg", fn="quantized_tanh", act_bits=3, out_store=STORE_I4,
                           why="packed I4 output: route_dense declines"))
            t.append(_case(s, xb, wk, wb, 9, K, units, bn="pos", fn="quantized_tanh", act_bits=8, out_store=STORE_I8,
                           why="packed I8 output: route_dense declines"))
    # ---- saturated operands.  8 bit at K = 4608: |sum| = 128 * 128 * 4608 = 75 497 472 ("min") and 127 * 127 * 4608 =
    #      74 322 432 ("max") > 2^24, so the int -> float conversion rounds; -128 * 127 * 4608 for "min_max"
    for fill in ("max", "min", "alternating", "min_max"):
        for units in (10, 65):
            t.append(_case(STORE_I8, 8, "quantized", 8, 5, 4608, units, fill=fill, why="saturated 8 x 8 bit, K = 4608"))
            t.append(_case(STORE_I4, 4, "quantized", 4, 5, 4608, units, fill=fill, why="saturated 4 x 4 bit, K = 4608"))
            t.append(_case(STORE_BIN, 1, "binary", 1, 5, 1000, units, fill=fill, why="saturated BIN at K = 1000 (pad bits)"))
            t.append(_case(STORE_BIN, 1, "binary", 1, 5, 100, units, fill=fill, why="saturated BIN at K = 100 (pad bits)"))
            t.append(_case(STORE_T2, 1, "ternary", 1, 5, 1000, units, fill=fill, why="saturated T2 at K = 1000"))
    # ---- float32 input (k_dense_f32in): cin % 4 == 0 and != 0, three kinds of input
    for cin in F32_CIN:
        for units in F32_UNITS:
            N = 3 if units == 1000 else 5
            t.append(_case(STORE_F32, 4, "quantized", 4, N, cin, units, bn="pos", xkind="grid",
                           why="float32 grid input, cin %% 4 = %d" % (cin % 4)))
            t.append(_case(STORE_F32, 0, "float", 0, N, cin, units, xkind="normal", bias=False,
                           why="float32 unit normal input"))
            t.append(_case(STORE_F32, 0, "float", 0, N, cin, units, xkind="cancel", bias=False,
                           why="float32 input built to cancel"))
    # grid-valued float32 input with every epilogue
    for cin in (63, 256):
        for xb, wk, wb in ((8, "quantized", 8), (2, "binary", 1), (3, "ternary", 1)):
            t.append(_case(STORE_F32, xb, wk, wb, 6, cin, 10, bias=False, why="f32 grid: no bias, no BN"))
            t.append(_case(STORE_F32, xb, wk, wb, 6, cin, 10, bn="neg", fn="binary_tanh", why="f32 grid: BN (gamma < 0), binary_tanh"))
            for nb in (2, 4, 8):
                t.append(_case(STORE_F32, xb, wk, wb, 6, cin, 10, bn="pos", fn="quantized_tanh", act_bits=nb,
                               why="f32 grid: quantized_tanh %d" % nb))
            t.append(_case(STORE_F32, xb, wk, wb, 6, cin, 10, bn="pos", res=True, why="f32 grid: float32 residual"))
            t.append(_case(STORE_F32, xb, wk, wb, 6, cin, 10, bn="pos", fn="quantized_tanh", act_bits=4, out_store=STORE_I4,
                           why="f32 grid: packed I4 output"))
    return t


def _random_dense_case(rng, seed):
    """One case of the random tail, drawn over the axes of the table (sizes log-uniform so that most cases are small)."""
    s = int(rng.choice([STORE_BIN, STORE_T2, STORE_I4, STORE_I8, STORE_F32]))
    K = int(np.exp(rng.uniform(0, np.log(8192)))) if rng.random() < 0.8 else int(rng.integers(1, 8193))
    units = int(np.exp(rng.uniform(0, np.log(1100)))) if rng.random() < 0.8 else int(rng.integers(1, 1101))
    N = int(rng.integers(1, 71))
    if s == STORE_BIN:
        xb, wk, wb = 1, "binary", 1
    elif s == STORE_T2:
        xb, (wk, wb) = 1, [("ternary", 1), ("binary", 1)][int(rng.integers(2))]
    else:
        top = 4 if s == STORE_I4 else 8
        xb = int(rng.integers(1, top + 1)) if s != STORE_F32 else int(rng.integers(2, 9))
        wk, wb = [("binary", 1), ("ternary", 1), ("quantized", int(rng.integers(2, top + 1)))][int(rng.integers(3))]
    bn = [None, "pos", "neg"][int(rng.integers(3))]
    fn, ab = [("none", 0), ("binary_tanh", 0), ("quantized_tanh", int(rng.choice([2, 3, 4, 8])))][int(rng.integers(3))]
    if fn != "none" and N * units < 16:
        N = 16                              # enough outputs for the CPU test to tell a degenerate case
    out_store = STORE_F32
    if fn != "none" and rng.random() < 0.25:
        out_store = STORE_BIN if fn == "binary_tanh" else (STORE_I4 if ab <= 4 else STORE_I8)
    return _case(s, xb, wk, wb, N, K, units, bias=bool(rng.random() < 0.7), bn=bn, fn=fn, act_bits=ab, out_store=out_store,
                 res=bool(rng.random() < 0.2), seed=seed, why="random tail")


RANDOM_TAIL = 220
_DENSE = None


def dense_cases():
    """The explicit table, then RANDOM_TAIL seeded random cases.  Every case gets a stable `id` and, unless it names one, a
    seed of its own."""
    global _DENSE
    if _DENSE is None:
        t = _dense_table()
        for i in range(RANDOM_TAIL):
            t.append(_random_dense_case(np.random.default_rng(70000 + i), 70000 + i))
        for i, c in enumerate(t):
            if not c["seed"]:
                c["seed"] = 1000 + i
            tags = [c["bn"], c["fn"][0] + str(c["act_bits"]) if c["fn"] != "none" else None, "res" if c["res"] else None,
                    "o" + STORE_NAME[c["out_store"]] if c["out_store"] != STORE_F32 else None,
                    c["fill"] or (c["xkind"] if c["x_store"] == STORE_F32 else None)]
            c["id"] = "-".join(["%03d-%s%d-%s%d-N%d-K%d-U%d" % (i, STORE_NAME[c["x_store"]], c["x_bits"], c["wkind"][0],
                                                                 c["wbits"], c["N"], c["K"], c["units"])] + [t_ for t_ in tags if t_])
        _DENSE = t
    return _DENSE


def _fill_pattern(fill, lo, hi, K, operand):
    """Codes along K of a saturated operand."""
    if fill == "max":
        return np.full(K, hi)
    if fill == "min":
        return np.full(K, lo)
    if fill == "alternating":
        return np.where(np.arange(K) % 2 == 0, hi, lo)
    assert fill == "min_max"
    return np.full(K, lo if operand == "x" else hi)


def _latent_kernel(c, rng):
    """The layer's latent float32 kernel (K, units).  Ternary kernels are drawn on a 2^-10 grid so that the cutoff's mean is
    exact in any summation order."""
    K, units = c["K"], c["units"]
    if c["fill"]:
        # latent +-1 quantizes to the top / bottom code of every quantizer (binarize, ternarize, quantize)
        col = _fill_pattern(c["fill"], -1.0, 1.0, K, "w").astype(F32)
        return np.repeat(col[:, None], units, axis=1)
    k = rng.uniform(-1, 1, (K, units))
    if c["wkind"] == "ternary":
        k = np.rint(k * 1024) / 1024
    return k.astype(F32)


def quantized_kernel(c, kernel):
    """The float32 values the layer multiplies with (the oracle's quantizers) and their integer codes * 2^-wshift."""
    if c["wkind"] == "binary":
        return O.binarize(kernel), 0
    if c["wkind"] == "ternary":
        return O._ternarize(kernel), 0
    if c["wkind"] == "quantized":
        return O.quantize(kernel, c["wbits"]), c["wbits"] - 1
    return kernel, None                     # float: used as is


def dense_inputs(c):
    """Everything a case feeds the layer with: activation codes / values, latent kernel, bias, BN parameters, residual."""
    rng = np.random.default_rng(c["seed"])
    N, K, units, s = c["N"], c["K"], c["units"], c["x_store"]
    d = {}
    if s == STORE_F32 and c["xkind"] != "grid":
        if c["xkind"] == "normal":
            x = rng.standard_normal((N, K)).astype(F32)
            kernel = rng.uniform(-1, 1, (K, units)).astype(F32)
        else:
            # x = [v0, -v0, v1, -v1, ...] against weights equal within each pair: the pairs cancel exactly in real numbers;
            # one small term (1e-6 of a typical product) is what is left, many orders below the terms
            v = rng.uniform(0.5, 2.0, (N, (K + 1) // 2)).astype(F32)
            x = np.stack([v, -v], axis=-1).reshape(N, -1)[:, :K].copy()
            wp = rng.uniform(0.5, 1.0, ((K + 1) // 2, units)).astype(F32)
            kernel = np.repeat(wp, 2, axis=0)[:K].copy()
            j = int(rng.integers(0, K))
            x[:, j ^ 1 if (j ^ 1) < K else j] = 0.0            # break one pair ...
            x[:, j] = (rng.uniform(1, 2, N) * 1e-6).astype(F32)  # ... and leave a small term in its place
            if K % 2 == 1 and j != K - 1:
                x[:, K - 1] = 0.0                                # the unpaired last element
        d["x"], d["codes"] = x, None
    else:
        bits = c["x_bits"]
        if c["fill"]:
            lo, hi = code_range(s, bits)
            codes = np.repeat(_fill_pattern(c["fill"], lo, hi, K, "x")[None, :], N, axis=0).astype(np.int8)
        else:
            codes = random_codes(rng, (N, K), s, bits)
        d["codes"] = codes
        d["x"] = (codes.astype(np.float64) * code_scale(s if s != STORE_F32 else STORE_I8, bits)).astype(F32)
        kernel = _latent_kernel(c, rng)
    d["kernel"] = kernel
    d["bias"] = (rng.standard_normal(units) * 0.05).astype(F32) if c["bias"] else None
    d["bn"] = None
    if c["bn"]:
        # pre-activations of K products of values in [-1, 1]: variance about K / 9 (1 for +-1 operands)
        var = max(1.0, K * (0.11 if s in (STORE_I4, STORE_I8, STORE_F32) else 0.6))
        if c["fill"]:
            var = float(K) ** 2
        gamma = rng.uniform(0.5, 1.5, units)
        d["bn"] = dict(op="bn", eps=1e-3, gamma=(gamma * (-1 if c["bn"] == "neg" else 1)).astype(F32),
                       beta=(rng.standard_normal(units) * 0.3).astype(F32),
                       mean=(rng.standard_normal(units) * 0.1 * np.sqrt(var)).astype(F32),
                       var=(var * rng.uniform(0.8, 1.25, units)).astype(F32))
    d["res"] = rng.standard_normal((N, units)).astype(F32) if c["res"] else None
    d["post_scale"] = 0.5 if c["res"] else 1.0
    return d


def dense_contraction(c, d):
    """The contraction alone, float32: an int64 matrix product of the integer codes, scaled by the (power of two) code
    scales and rounded once; float32 inputs that are not on a grid: a float64 matrix product, rounded once."""
    wq, wshift = quantized_kernel(c, d["kernel"])
    if d["codes"] is not None and wshift is not None:
        wcodes = np.rint(wq.astype(np.float64) * 2.0 ** wshift).astype(np.int64)
        assert np.array_equal(wcodes * 2.0 ** -wshift, wq.astype(np.float64))
        acc = d["codes"].astype(np.int64) @ wcodes
        store = c["x_store"] if c["x_store"] != STORE_F32 else STORE_I8
        return (acc.astype(np.float64) * (code_scale(store, c["x_bits"]) * 2.0 ** -wshift)).astype(F32)
    return (d["x"].astype(np.float64) @ wq.astype(np.float64)).astype(F32)


def dense_epilogue(c, d, v):
    """What the launch fuses behind the contraction, in the ABI's order, in the oracle's float32 operations."""
    if d["bias"] is not None:
        v = O.bias_add(v, d["bias"])
    if d["bn"] is not None:
        b = d["bn"]
        v = O.batchnorm_inference(v, b["gamma"], b["beta"], b["mean"], b["var"], b["eps"])
    if d["res"] is not None:
        v = ((d["res"] + v).astype(F32) * F32(d["post_scale"])).astype(F32)
    if c["fn"] == "binary_tanh":
        v = O.binary_tanh(v)
    elif c["fn"] == "quantized_tanh":
        v = O.quantized_tanh(v, c["act_bits"])
    return v


def dense_reference(c, d=None):
    """Expected float32 output (N, units) of a case; a packed output holds the codes of these values."""
    d = dense_inputs(c) if d is None else d
    return dense_epilogue(c, d, dense_contraction(c, d))


def dense_f32_bound(c, d):
    """For float32 inputs off the grid: (s, bound) with s the float64 dot products and
    bound = ulp32(s) + K * 2^-53 * sum_k |x_k w_k|: one rounding to float32, plus the worst-case error of K float64
    additions in any order."""
    wq, _ = quantized_kernel(c, d["kernel"])
    x64, w64 = d["x"].astype(np.float64), wq.astype(np.float64)
    s = x64 @ w64
    mag = np.abs(x64) @ np.abs(w64)
    return s, ulp32(s) + c["K"] * 2.0 ** -53 * mag


def ulp32(v):
    """Spacing of float32 at the float32 nearest to v (the smallest denormal at 0)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(F32)).astype(np.float64)


def out_codes(c, values):
    """Integer codes of a packed output (values of dense_reference)."""
    if c["out_store"] == STORE_BIN or c["fn"] == "binary_tanh":
        return np.rint(values).astype(np.int64)
    return np.rint(values.astype(np.float64) * 2.0 ** (c["act_bits"] - 1)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# average pool
# ---------------------------------------------------------------------------------------------------------------------
def avgpool_wave(c):
    """The condition under which qnn_avgpool_packed_f32 launches k_avgpool_i4_wave."""
    return c["store"] == STORE_I4 and c["C"] % 64 == 0 and c["size"] * c["size"] >= 8


def avgpool_cases():
    t = []

    def add(store, bits, N, H, W, C, size, why, fill=None):
        t.append(dict(store=store, bits=bits, N=N, H=H, W=W, C=C, size=size, fill=fill, why=why, seed=500 + len(t)))

    # (i) the wave kernel: bits 2, 3 (and 4) in I4 storage, C in {64, 192, 512}, H and W not multiples of `size`
    for bits in (2, 3, 4):
        for C in (64, 192, 512):
            for size, H, W in ((3, 10, 11), (4, 9, 14), (7, 15, 9), (8, 17, 12)):
                add(STORE_I4, bits, 2, H, W, C, size, "wave kernel, remainder rows / columns dropped")
    for bits in (2, 3, 4):
        add(STORE_I4, bits, 3, 7, 7, 64, 7, "wave kernel, global 7 x 7 pool (ImageNet ResNet)")
        add(STORE_I4, bits, 3, 8, 8, 64, 8, "wave kernel, global 8 x 8 pool (CIFAR ResNet)")
        add(STORE_I4, bits, 2, 8, 8, 512, 8, "wave kernel, global 8 x 8 pool, 512 channels")
    # (ii) one condition short of the wave kernel each
    add(STORE_I4, 3, 2, 9, 10, 48, 3, "C = 48: not a multiple of 64")
    add(STORE_I4, 2, 2, 9, 10, 64, 2, "size 2: a window of 4 < 8 pixels")
    add(STORE_I8, 3, 2, 9, 10, 64, 3, "I8 storage")
    add(STORE_I8, 8, 2, 16, 16, 64, 8, "I8 storage, 8 bit")
    add(STORE_BIN, 1, 2, 9, 10, 64, 3, "BIN storage")
    add(STORE_BIN, 1, 2, 8, 8, 33, 8, "BIN storage, pad bits")
    add(STORE_I4, 4, 2, 5, 6, 5, 2, "C = 5: pad fields")
    # (iii) the generic kernel's grid-stride loop: its grid is capped at 65535 blocks of 256 threads = 16 776 960 outputs;
    #       N = 35, 64 x 64, C = 120, size 1 gives 35 * 64 * 64 * 120 = 17 203 200 outputs, so 426 240 of them are computed
    #       in the second turn of the loop
    add(STORE_I8, 8, 35, 64, 64, 120, 1, "17 203 200 outputs > 65535 * 256: the grid-stride loop wraps")
    # (iv) saturated codes: every code at the most negative value
    add(STORE_I4, 4, 2, 16, 16, 64, 8, "saturated, wave kernel", fill="min")
    add(STORE_I4, 2, 2, 16, 16, 64, 8, "saturated 2 bit, wave kernel", fill="min")
    add(STORE_I8, 8, 2, 16, 16, 24, 8, "saturated 8 bit, generic kernel", fill="min")
    add(STORE_BIN, 1, 2, 16, 16, 64, 8, "saturated BIN", fill="min")
    for c in t:
        c["id"] = "%s%d-%dx%dx%dx%d-s%d%s" % (STORE_NAME[c["store"]], c["bits"], c["N"], c["H"], c["W"], c["C"], c["size"],
                                              "-min" if c["fill"] else "")
    return t


def avgpool_codes(c):
    rng = np.random.default_rng(c["seed"])
    shape = (c["N"], c["H"], c["W"], c["C"])
    if c["fill"] == "min":
        return np.full(shape, code_range(c["store"], c["bits"])[0], dtype=np.int8)
    return random_codes(rng, shape, c["store"], c["bits"])


def avgpool_reference(c, codes):
    """Window sums of the codes in int64 -> float64 value (exact) -> float32 (exact) -> one float32 division."""
    N, H, W, C, size = c["N"], c["H"], c["W"], c["C"], c["size"]
    Ho, Wo = H // size, W // size
    win = codes[:, :Ho * size, :Wo * size, :].reshape(N, Ho, size, Wo, size, C)
    acc = win.sum(axis=(2, 4), dtype=np.int64)
    s = (acc.astype(np.float64) * code_scale(c["store"], c["bits"])).astype(F32)
    return (s / F32(size * size)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# softmax
# ---------------------------------------------------------------------------------------------------------------------
SOFTMAX_COLS = (1, 2, 10, 255, 256, 257, 1000, 4099)
SOFTMAX_ROWS = (1, 3, 300, 5000)
SOFTMAX_KINDS = ("normal6", "one_hot80", "equal", "spread1400", "tiny")


def softmax_cases():
    return [dict(rows=r, cols=c, kind=k, seed=900 + 7 * i, id="%dx%d-%s" % (r, c, k))
            for i, (r, c, k) in enumerate((r, c, k) for r in SOFTMAX_ROWS for c in SOFTMAX_COLS for k in SOFTMAX_KINDS)]


def softmax_logits(c):
    """Finite float32 logits (non-finite ones are out of scope).  normal6: normal * 6; one_hot80: one logit 80 above normal
    ones; equal: all equal; spread1400: uniform over [-1400, 0], so most terms underflow in float64 after the shift (exp
    underflows below -745); tiny: one logit at 0 and the rest in [-92, -18.5]: probabilities between 1e-40 and 1e-8,
    float32 denormals (below 1.2e-38) included."""
    rng = np.random.default_rng(c["seed"])
    rows, cols, kind = c["rows"], c["cols"], c["kind"]
    if kind == "normal6":
        x = rng.standard_normal((rows, cols)) * 6
    elif kind == "one_hot80":
        x = rng.standard_normal((rows, cols))
        x[np.arange(rows), rng.integers(0, cols, rows)] += 80.0
    elif kind == "equal":
        x = np.repeat(rng.standard_normal((rows, 1)) * 50, cols, axis=1)
    elif kind == "spread1400":
        x = rng.uniform(-1400, 0, (rows, cols)) + rng.standard_normal((rows, 1)) * 100
    else:
        x = rng.uniform(-92, -18.5, (rows, cols))
        x[np.arange(rows), rng.integers(0, cols, rows)] = 0.0
    return x.astype(F32)


def softmax_reference(x):
    """The float64 definition, max-shifted, rounded once."""
    z = x.astype(np.float64)
    z = z - z.max(axis=-1, keepdims=True)
    e = np.exp(z)
    return (e / e.sum(axis=-1, keepdims=True)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# pack / unpack
# ---------------------------------------------------------------------------------------------------------------------
PACK_PIXELS = (1, 63, 64, 65, 4097, 100003)
PACK_CHANNELS = (1, 3, 31, 32, 33, 64, 65, 200, 256, 512)
PACK_FORMATS = ((STORE_BIN, 1), (STORE_I4, 2), (STORE_I4, 3), (STORE_I4, 4), (STORE_I8, 5), (STORE_I8, 8), (STORE_T2, 1))


def pack_cases():
    return [dict(store=s, bits=b, pixels=p, C=C, seed=300 + i, id="%s%d-%dx%d" % (STORE_NAME[s], b, p, C))
            for i, (s, b, p, C) in enumerate((s, b, p, C) for s, b in PACK_FORMATS for p in PACK_PIXELS for C in PACK_CHANNELS)]


def pack_codes(c):
    """Random codes (pixels, C); I4 / I8 codes span the whole range of `bits`, both extremes present whenever C * pixels
    allows."""
    rng = np.random.default_rng(c["seed"])
    if c["store"] in (STORE_I4, STORE_I8):
        lo, hi = code_range(c["store"], c["bits"])
        codes = rng.integers(lo, hi + 1, (c["pixels"], c["C"])).astype(np.int8)
        flat = codes.reshape(-1)
        flat[0] = lo
        flat[-1] = hi if flat.size > 1 else lo
        return codes
    return random_codes(rng, (c["pixels"], c["C"]), c["store"], c["bits"])


def pack_values(c, codes):
    return (codes.astype(F32) * F32(code_scale(c["store"], c["bits"]))).astype(F32)


def pad_field_mask(store, C):
    """uint32 mask per word of a pixel (words(store, C),): the bits that belong to pad fields and must be zero."""
    pw = per_word(store)
    bits = 32 // pw
    cw = -(-C // pw)
    m = np.zeros(cw, dtype=np.uint32)
    used = C - (cw - 1) * pw
    if used < pw:
        m[-1] = np.uint32((0xffffffff << (used * bits)) & 0xffffffff)
    return np.repeat(m, 2) if store == STORE_T2 else m


# ---------------------------------------------------------------------------------------------------------------------
# elementwise activations
# ---------------------------------------------------------------------------------------------------------------------
def _source_constant(pattern):
    """The groups of `pattern` in csrc/qnn_elementwise.hip, as integers."""
    with open(os.path.join(CSRC, "qnn_elementwise.hip")) as f:
        m = re.search(pattern, f.read())
    assert m is not None, pattern
    return [int(g) for g in m.groups()]


ACT_UNROLL, = _source_constant(r"#define QNN_ACT_UNROLL\s+(\d+)")
_one, _shift = _source_constant(r"constexpr int kMaxBlocks = (\d+) << (\d+);")
ACT_MAX_BLOCKS = _one << _shift
# act_grid caps the launch at kMaxBlocks blocks of 256 threads of one float4 each: the strided loop of k_act_f32 wraps
# only above this many elements.  At kMaxBlocks = 2^22 that is 2^32 elements = 16 GiB of float32 per tensor, beyond the
# 2 GiB this suite allocates at most: the wrapping length is therefore NOT in the table (stated here instead of skipped at
# run time).  A smaller cap in the source puts it back.
ACT_WRAP_LENGTH = ACT_MAX_BLOCKS * 256 * 4 + 5
ACT_WRAP_TESTABLE = ACT_WRAP_LENGTH * 4 <= (1 << 31)
ACT_LENGTHS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 4 * 256 * ACT_UNROLL + 3) + ((ACT_WRAP_LENGTH,) if ACT_WRAP_TESTABLE else ())
ACT_OFFSETS = (0, 1, 2, 3)
ACT_FNS = (("binary_tanh", 0), ("quantized_tanh", 2), ("quantized_tanh", 3), ("quantized_tanh", 4), ("quantized_tanh", 8),
           ("quantized_tanh", 16))


def edge_values():
    """Signed zeros, the 2^-24 neighbourhood of binary_tanh's threshold, clip points, grid points and large values."""
    e = [0.0, -0.0, 2.0 ** -24, 2.0 ** -23, -2.0 ** -24, 2.0 ** -25, 1e-9, -1e-9, 1e-45, -1e-45, 0.5, -0.5, 1.0, -1.0,
         0.0625, 0.1875, 0.3125, 0.4375, 0.9375, 0.96875, -0.0625, -0.1875, -0.3125, -0.9375, -1.2, 1.2, 1e30, -1e30]
    return np.array(e, dtype=F32)


def act_values(n, nb, seed):
    """n float32 values: the edge values, the half-way points (k + 0.5) / 2^(nb-1) of the grid (all of them up to 8 bit, a
    spread of 4096 for 16 bit) and their float32 neighbours, then uniform values in [-1.3, 1.3]; shuffled so that short
    lengths see special values too."""
    rng = np.random.default_rng(seed)
    m = 2.0 ** (max(nb, 1) - 1)
    k = np.arange(-m - 1, m + 1) if nb <= 8 else np.concatenate([np.arange(-m - 1, -m + 1024), np.arange(-1024, 1024),
                                                                   np.arange(m - 1024, m + 1)])
    half = ((k + 0.5) / m).astype(F32)
    pool = np.concatenate([edge_values(), half, np.nextafter(half, F32(2)), np.nextafter(half, F32(-2)), (k / m).astype(F32)])
    rng.shuffle(pool)
    if n <= pool.size:
        return pool[:n].copy()
    return np.concatenate([pool, rng.uniform(-1.3, 1.3, n - pool.size).astype(F32)])


def act_reference(fn, nb, x):
    return O.binary_tanh(x) if fn == "binary_tanh" else O.quantized_tanh(x, nb)


TERNARY_LENGTHS = (1, 2, 63, 64, 65, 10 ** 6 + 1)


def ternary_threshold_tensor(n, seed):
    """A tensor whose mean(|x|) is exactly 0.5, so that ternary_tanh's cutoff is t = float32(0.7) * 0.5 exactly, with 32
    elements at |x| = t (16 at +t -> 0: not above the cutoff; 16 at -t -> -1: `<= -cutoff`).  All values are multiples of
    2^-25 below 2, so the sum is exact in float64 in any order.  Layout: 32 elements at +-t, 16 at 0.5 + d (d = 2 * (0.5 -
    t), making up for the 32 that sit below 0.5), the rest half at +-1 and half at 0 (mean 0.5) in a seeded shuffle."""
    assert n >= 64 and (n - 48) % 2 == 0
    t = F32(F32(0.7) * F32(0.5))
    d = 2.0 * (0.5 - float(t))
    up = F32(0.5 + d)
    assert float(up) == 0.5 + d and float(up) <= 1.0
    rng = np.random.default_rng(seed)
    rest = n - 48
    x = np.concatenate([np.full(16, t), np.full(16, -t), np.full(16, up),
                        np.where(rng.random(rest // 2) < 0.5, F32(1), F32(-1)), np.zeros(rest // 2)]).astype(F32)
    rng.shuffle(x)
    from fractions import Fraction
    if n <= 4096:
        assert sum(Fraction(float(abs(v))) for v in x) == Fraction(n, 2)
    return x, t
