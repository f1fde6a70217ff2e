"""Packed codes plus a device-resident scale (include/qnn_abi_scaled.h), restated in numpy on top of maxrelu_cases.py: the
integer codes of quantized_maxrelu / quantized_leakymaxrelu and their word layout per store, the integer reference of a
scaled conv / dense call (int64 accumulation of activation codes x weight codes, times scale * P, then the oracle's
epilogue), the exactness rule that says when that equals the float32 route bit for bit, and the conv / dense cases the
GPU tests run.  test_scaled_cpu.py holds all of it against maxrelu_cases.maxact and the oracle's float convolution."""
import numpy as np

import maxrelu_cases as C
from oracle import qnn_oracle as O

F32 = np.float32
STORE_I4, STORE_I8 = 4, 8


# ---- the codes and their layout --------------------------------------------------------------------------------------
def codes(x, nb, fn, M):
    """code = clip(rint(L(x) * m / P), lo, m - 1) as int64, P from the maximum M (qnn_abi_maxact.h, to the letter); all
    zero for an M outside the exact range."""
    assert fn in C.FNS
    x = np.asarray(x, dtype=F32)
    e = C.scale_exponent(M)
    if e is None:
        return np.zeros(x.shape, dtype=np.int64)
    m = F32(2.0 ** (nb - 1))
    v, lo = (x, F32(0)) if fn == "quantized_maxrelu" else (C.leaky(x), -m)
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.clip(np.rint((v * F32(2.0 ** (nb - 1 - e))).astype(F32)), lo, m - F32(1))
    return c.astype(np.int64)


def values(k, nb, M):
    """code * P / m as float32 (exact: a small integer times a power of two); NaN for an M outside the exact range."""
    e = C.scale_exponent(M)
    if e is None:
        return np.full(np.shape(k), np.nan, dtype=F32)
    return (np.asarray(k, dtype=np.float64) * 2.0 ** (e - (nb - 1))).astype(F32) + F32(0)


def per_word(store):
    return {STORE_I4: 8, STORE_I8: 4}[store]


def pack_words(k, store):
    """(pixels, channels) integer codes -> (pixels, ceil(channels / per_word)) uint32 words in qnn_pack_f32's layout: field j
    of a word is bits [j * w, (j + 1) * w), w = 32 / per_word; codes sign-extended into their field; spare fields zero."""
    k = np.asarray(k, dtype=np.int64)
    pixels, ch = k.shape
    pw = per_word(store)
    bits = 32 // pw
    cw = (ch + pw - 1) // pw
    padded = np.zeros((pixels, cw * pw), dtype=np.int64)
    padded[:, :ch] = k & ((1 << bits) - 1)
    out = np.zeros((pixels, cw), dtype=np.int64)
    for j in range(pw):
        out |= padded[:, j::pw] << (j * bits)
    return out.astype(np.uint32)


def spare_mask(ch, store):
    """Mask of the bits of a pixel's LAST word that lie beyond channel ch - 1 (0 when the channels fill the word)."""
    pw = per_word(store)
    used = ch % pw
    return 0 if used == 0 else (0xFFFFFFFF << (used * (32 // pw))) & 0xFFFFFFFF


# ---- the exactness rule ----------------------------------------------------------------------------------------------
def weight_bits(op):
    return int(op["nb"]) if op["kind"] == "quantized" else 1


def contraction_depth(op):
    k = np.asarray(op["kernel"]).shape
    return int(np.prod(k[:-1]))


def route_is_exact(K, nb, wbits):
    """The float32 route's fmaf chain over K products of an nb-bit activation code and a wbits-bit weight code is exact --
    hence equal to the integer route bit for bit -- when every partial sum fits 24 bits: K * 2^(nb-1) * 2^(wbits-1) <= 2^24
    (wbits = 1 for binary and ternary weights)."""
    return K * 2 ** (nb - 1) * 2 ** (wbits - 1) <= 2 ** 24


# ---- the scaled consumers ----------------------------------------------------------------------------------------------
def _dilated(w, d):
    """HWIO kernel with d - 1 zero taps between neighbours: the dilated window as an ordinary one (a zero tap adds nothing,
    in the integer sum and in an fma chain alike)."""
    if d == 1:
        return w
    kh, kw, ci, co = w.shape
    out = np.zeros((d * (kh - 1) + 1, d * (kw - 1) + 1, ci, co), dtype=w.dtype)
    out[::d, ::d] = w
    return out


def quantized_kernel(op):
    """The float32 weights the layer contracts with (oracle: binarize / ternarize / quantize)."""
    if op["kind"] == "binary":
        return O.binarize(op["kernel"], op.get("H", 1.0))
    if op["kind"] == "ternary":
        return O._ternarize(op["kernel"], op.get("H", 1.0))
    return O.quantize(op["kernel"], op["nb"])


def epilogue(v, op, bn=None, res=None, post_scale=1.0, trick=None):
    """What follows the contraction, in the reference's op order (oracle functions): identity trick, bias, BN, float32
    residual merge (res + v) * post_scale."""
    v = np.asarray(v, dtype=F32)
    with np.errstate(invalid="ignore"):
        if trick is not None:
            v = O._trick(v, F32(trick[0]), F32(trick[1]))
        if op.get("bias") is not None:
            v = O.bias_add(v, op["bias"])
        if bn is not None:
            v = O.batchnorm_inference(v, bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"])
        if res is not None:
            v = ((np.asarray(res, dtype=F32) + v).astype(F32) * F32(post_scale)).astype(F32)
    return v


def scaled_reference(k, nb, M, op, **epi):
    """The contract of qnn_conv2d_forward_scaled / qnn_dense_forward_scaled: int64 sum of activation codes k (NHWC, or
    (N, K) for a dense op) x weight codes, as float32, times scale * P (scale = 2^-(wshift + nb - 1); both powers of two),
    then the epilogue.  NaN everywhere in front of the epilogue for an M outside the exact range."""
    wc, wshift = O.weight_codes(op)
    if op["op"] == "dense":
        acc = np.asarray(k, dtype=np.int64).dot(wc.reshape(-1, wc.shape[-1]))
    else:
        d = int(op.get("dilation_rate", 1))
        acc = O.int_conv2d(k, _dilated(wc, d), tuple(op["strides"]), op["padding"])
    assert np.abs(acc).max() <= 2 ** 24
    e = C.scale_exponent(M)
    if e is None:
        v = np.full(acc.shape, np.nan, dtype=F32)
    else:
        v = (acc.astype(F32).astype(np.float64) * 2.0 ** (e - wshift - (nb - 1))).astype(F32)
    return epilogue(v, op, **epi)


def float_reference(y, op, order="ideal", **epi):
    """The float32 route on the float32 activation y = code * P / m: the oracle's float convolution ("ideal": float64
    accumulation, one rounding; "device": the kernels' fma chain) of y with the layer's quantised weights, then the same
    epilogue."""
    wq = quantized_kernel(op)
    if op["op"] == "dense":
        if order == "device":
            v = O.conv2d_device_order(np.asarray(y, F32)[:, None, None, :], wq.reshape(1, 1, *wq.shape), (1, 1), "valid")[:, 0, 0]
        else:
            v = O.dot(y, wq)
    else:
        wd = _dilated(wq, int(op.get("dilation_rate", 1)))
        conv = O.conv2d_device_order if order == "device" else O.conv2d
        v = conv(y, wd, tuple(op["strides"]), op["padding"])
    return epilogue(v, op, **epi)


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------
def _op(kind, wnb, kh, cin, cout, stride, padding, seed, dilation=1, bias=True):
    rng = np.random.default_rng(seed)
    op = {"op": "conv", "kind": kind, "kernel": rng.uniform(-1.0, 1.0, (kh, kh, cin, cout)).astype(F32),
          "bias": (rng.standard_normal(cout) * 0.05).astype(F32) if bias else None, "strides": (stride, stride),
          "padding": padding}
    if kind == "quantized":
        op["nb"] = wnb
    if dilation != 1:
        op["dilation_rate"] = dilation
    return op


def _dense(kind, wnb, cin, cout, seed):
    rng = np.random.default_rng(seed)
    op = {"op": "dense", "kind": kind, "kernel": rng.uniform(-1.0, 1.0, (cin, cout)).astype(F32),
          "bias": (rng.standard_normal(cout) * 0.05).astype(F32)}
    if kind == "quantized":
        op["nb"] = wnb
    return op


# name -> (op, input shape, activation bits, store, kernel expected, epilogue pieces the route's capability list admits)
CONSUMERS = {
    # route_generic: 8 input channels, a 3x3 stride-2 'valid' window (qnn_prepack_weights takes no window above 3x3, so the
    # 5x5 form of this case does not exist in the library); and a dilated 3x3
    "generic_3x3_s2_valid": (_op("quantized", 4, 3, 8, 12, 2, "valid", 61), (2, 11, 13, 8), 4, STORE_I4, "generic_scaled",
                             ("bn", "res", "trick")),
    "generic_dilated": (_op("quantized", 4, 3, 8, 8, 1, "same", 62, dilation=2), (2, 7, 9, 8), 4, STORE_I4, "generic_scaled",
                        ("bn", "res", "trick")),
    "generic_i8": (_op("quantized", 8, 3, 12, 8, 1, "same", 63), (2, 6, 7, 12), 8, STORE_I8, "generic_scaled",
                   ("bn", "res", "trick")),
    "generic_binary_w": (_op("binary", 1, 3, 8, 8, 1, "same", 64), (2, 6, 7, 8), 4, STORE_I4, "generic_scaled",
                         ("bn", "res", "trick")),
    # qnn_route_gemm: the smallest shapes its scaled form takes (64 input channels, 128 filters = the 256 x 128 tile; 256
    # filters = the 256 x 256 tile), N = 2, H = 7, W = 20: 280 pixels, one whole 256-pixel tile and a ragged one.  The
    # route lists neither the residual merge for these kernels nor the trick.
    "gemm_i4_128": (_op("quantized", 4, 3, 64, 128, 1, "same", 91), (2, 7, 20, 64), 4, STORE_I4, "mfma_i4_256x128_scaled", ("bn",)),
    "gemm_i4_256": (_op("quantized", 4, 3, 64, 256, 1, "same", 92), (2, 7, 20, 64), 4, STORE_I4, "mfma_i4_256x256_scaled", ("bn",)),
    "gemm_i8_128": (_op("quantized", 8, 3, 64, 128, 1, "same", 93), (2, 7, 20, 64), 8, STORE_I8, "mfma_i8_256x128_scaled", ("bn",)),
    "gemm_i8_256": (_op("quantized", 8, 3, 64, 256, 1, "same", 94), (2, 7, 20, 64), 8, STORE_I8, "mfma_i8_256x256_scaled", ("bn",)),
    # 16 / 32 / 64 channels on the strip-shaped image (N = 2, H = 7, W = 20: one whole 16-column strip and a ragged one), int4
    # and int8: no strip kernel has a float32 output, so today such a scaled call runs on k_conv_generic; a strip route for
    # scaled calls will show up here as a deliberate change of the kernel name
    "c16_i4": (_op("quantized", 4, 3, 16, 16, 1, "same", 95), (2, 7, 20, 16), 4, STORE_I4, "generic_scaled", ("bn", "res")),
    "c32_i4": (_op("quantized", 4, 3, 32, 32, 1, "same", 96), (2, 7, 20, 32), 4, STORE_I4, "generic_scaled", ("bn", "res")),
    "c64_i4": (_op("quantized", 4, 3, 64, 64, 1, "same", 97), (2, 7, 20, 64), 4, STORE_I4, "generic_scaled", ("bn", "res")),
    "c32_i8": (_op("quantized", 8, 3, 32, 32, 1, "same", 98), (2, 7, 20, 32), 8, STORE_I8, "generic_scaled", ("bn", "res")),
    # route_dense: 6 x 64 -> 10 (the split kernel at I8: 16 words; the one-thread form at I4: 8 words), no residual, no trick
    "dense_i4": (_dense("quantized", 4, 64, 10, 65), (6, 64), 4, STORE_I4, "dense_i4_scaled", ("bn",)),
    "dense_i8": (_dense("quantized", 8, 64, 10, 66), (6, 64), 8, STORE_I8, "dense_i8_scaled", ("bn",)),
    "dense_wide_store": (_dense("quantized", 8, 64, 10, 67), (6, 64), 4, STORE_I8, "dense_i8_scaled", ("bn",)),
    "dense_70_units": (_dense("quantized", 4, 32, 70, 68), (5, 32), 4, STORE_I4, "dense_i4_scaled", ("bn",)),
}
SCALES = (2.0 ** -3, 1.0, 2.0 ** 5)          # P of the ordinary runs; one bare run each at 2^-64 and 2^64


def consumer_input(name, P, fn="quantized_leakymaxrelu", seed=0):
    """(x float32, M) for case `name`: values over both clips of the activation, the maximum M = P (1 - 2^-10) in the
    tensor (so that P is the scale and M itself clips at the top code) -- every other value is below it."""
    op, shape, nb, store, kernel, pieces = CONSUMERS[name]
    rng = np.random.default_rng(1000 + seed + sum(map(ord, name)))
    M = F32(P * (1.0 - 2.0 ** -10))
    x = np.minimum((rng.uniform(-12.0, 1.0, shape) * float(P)).astype(F32), M)
    x.reshape(-1)[3] = M
    return x, M


def epilogue_sets(pieces):
    """bare, then every piece the route admits: bias + BN, a float32 residual with post_scale 0.5, the identity trick."""
    sets = [()]
    if "bn" in pieces:
        sets.append(("bn",))
    if "res" in pieces:
        sets.append(("bn", "res"))
    if "trick" in pieces:
        sets.append(("trick",))
    return sets


def epilogue_args(name, which, out_shape, P):
    """numpy epilogue arguments of case `name` for the piece set `which`; the residual is of the output's magnitude."""
    op = CONSUMERS[name][0]
    cout = op["kernel"].shape[-1]
    epi = {}
    if "bn" in which:
        rng = np.random.default_rng(77)
        epi["bn"] = {"op": "bn", "gamma": rng.uniform(0.5, 1.5, cout).astype(F32) * np.where(np.arange(cout) % 2, -1, 1).astype(F32),
                     "beta": np.linspace(-1.0, 1.0, cout).astype(F32), "mean": (rng.standard_normal(cout) * 0.1).astype(F32),
                     "var": rng.uniform(0.8, 1.25, cout).astype(F32), "eps": 1e-3}
    if "res" in which:
        epi["res"] = (np.random.default_rng(78).standard_normal(out_shape) * float(P)).astype(F32)
        epi["post_scale"] = 0.5
    if "trick" in which:
        k = op["kernel"].shape
        klm = O.glorot_klm(*k)
        c_in, s_in, c_out, s_out = O.trick_constants(klm, "nep50")
        epi["trick"] = (float(c_out), float(s_out))
    return epi


def beyond_the_bound():
    """A dense case just beyond the rule, every activation code and every weight code at its largest (127 each, 8 / 8 bits),
    in which the float32 route and the integer route differ: the partial sums j * 16129 pass 2^24 at j = 1041, and
    1041 * 16129 is odd, so no float32 holds it.  (The rule's bound, K <= 1024, is the last K at which even the products
    of the clip edges -128 * -128 = 2^14 cannot reach 2^24.)  Returns (codes, op, nb, M)."""
    K, nb = 1041, 8
    op = {"op": "dense", "kind": "quantized", "nb": 8, "kernel": np.full((K, 1), 1.0, dtype=F32), "bias": None}
    k = np.full((1, K), 2 ** (nb - 1) - 1, dtype=np.int64)
    return k, op, nb, F32(1.0)
