"""Cases and the numpy reference of the merge tests (test_merge_cpu.py, test_gpu_merge.py): Keras' Add / Subtract / Multiply /
Average / Maximum / Minimum on float32 tensors and on packed codes, as include/qnn_abi_merge.h states them.

  OPS, CHANNELS, PIXELS, BITS, NS, AVG_NS   the ops, the channel counts per store, the pixel counts, the code widths, the
                                            numbers of inputs
  out_kind                                  the table: which (op, store) pairs leave codes and which float32
  words / encode / decode / spare           the layout qnn_pack_f32 writes, vectorised; test_merge_cpu.py holds them against
                                            concat_cases' channel-by-channel restatement
  codes / values                            integer codes with both extreme codes in every tensor, and their float32 values
  ref_f32 / ref_codes                       the float32 chain (np.float32 division for avg) and the rules on integer codes
  f32_inputs / special_inputs               float32 operands with magnitudes in 2^-20 .. 2^20 whose every partial result is
                                            zero or normal (checked), and the inf / NaN / equal / +-0 pairs of max and min
  same_f32                                  bit for bit, NaN for NaN; optionally a zero for a zero of either sign

Plain numpy: neither torch nor the package is imported here."""
import functools
import zlib

import numpy as np

F32 = np.float32
STORE = {"f32": 0, "bin": 1, "t2": 2, "i4": 4, "i8": 8}                  # include/qnn_abi.h
PER_WORD = {"bin": 32, "t2": 32, "i4": 8, "i8": 4}
OPS = ("add", "sub", "mul", "avg", "max", "min")
OP_CODE = {op: i for i, op in enumerate(OPS)}                           # QNN_MERGE_*
MAX_INPUTS = 8                                                          # QNN_MERGE_MAX

CHANNELS = {"bin": (3, 32, 33, 128), "i4": (5, 8, 12, 64), "i8": (3, 4, 6, 16), "t2": (3, 32, 33), "f32": (1, 3, 4, 7)}
PIXELS = (1, 5, 64, 257, 2051)           # 2051: more than one 256-thread block and a tail in every form
BITS = {"bin": (1,), "t2": (1,), "i4": (2, 3, 4), "i8": (5, 8), "f32": (0,)}
NS = (2, 3, 8)
AVG_NS = (3, 5, 6, 7)


def ns_of(op):
    return (2,) if op == "sub" else NS


def out_kind(op, kind):
    """The store of the result: `kind` itself where it is again a code, "f32" otherwise (qnn_merge_out_store)."""
    assert op in OPS and kind in STORE
    if kind == "f32" or op in ("max", "min") or (op == "mul" and kind in ("bin", "t2")):
        return kind
    return "f32"


PACKED_OUT = [(op, kind) for op in OPS for kind in ("bin", "i4", "i8", "t2") if out_kind(op, kind) == kind]
F32_OUT = [(op, kind) for op in OPS for kind in ("bin", "i4", "i8", "t2") if out_kind(op, kind) == "f32"]


def form(op, kind, C, pixels, aligned16=True):
    """The kernel form of include/qnn_abi_merge.h / csrc/qnn_merge.hip for one call, restated from the host's rule: 16
    (16 bytes per lane) where every pointer is 16-byte aligned and, for float32 and for codes -> codes, the tensor is a
    flat run of whole words (no spare bits in a row's last word) whose number divides by 4; for codes -> float32, the
    channels divide by 4.  4 (one value, word, word pair or channel per lane) otherwise."""
    if not aligned16:
        return 4
    if kind != "f32" and out_kind(op, kind) == "f32":
        return 16 if C % 4 == 0 else 4
    whole = kind == "f32" or C % PER_WORD[kind] == 0
    return 16 if whole and (pixels * words(kind, C)) % 4 == 0 else 4


# ---- the packed layout -----------------------------------------------------------------------------------------------------
def words(kind, C):
    """Words of one row: ceil(C / per_word); T2: a (mask, sign) word pair per 32 channels; float32: C."""
    if kind == "f32":
        return C
    n = -(-C // PER_WORD[kind])
    return 2 * n if kind == "t2" else n


def _fields(plane, pw, field):
    """(P, C) non-negative field values -> (P, ceil(C / pw)) uint32 words, channel c at bit (c % pw) * field of word c // pw."""
    P, C = plane.shape
    n = -(-C // pw)
    padded = np.zeros((P, n * pw), dtype=np.uint64)
    padded[:, :C] = plane
    sh = (np.arange(pw, dtype=np.uint64) * np.uint64(field))
    return (padded.reshape(P, n, pw) << sh).sum(axis=-1).astype(np.uint32)


def encode(k, kind):
    """Codes (P, C) -> uint32 words (P, words(kind, C)): two's complement in the field; bin: bit = 1 <=> +1; t2: the mask
    word (code != 0) then the sign word (code > 0) of each 32 channels.  Spare bits zero."""
    k = np.asarray(k, dtype=np.int64)
    pw = PER_WORD[kind]
    field = 32 // pw
    if kind == "bin":
        return _fields((k > 0).astype(np.uint64), pw, 1)
    if kind == "t2":
        m, s = _fields((k != 0).astype(np.uint64), 32, 1), _fields((k > 0).astype(np.uint64), 32, 1)
        return np.stack([m, s], axis=-1).reshape(k.shape[0], -1)
    return _fields((k & ((1 << field) - 1)).astype(np.uint64), pw, field)


def decode(w, kind, C):
    """The inverse of encode on the C channels of every row; the spare bits are not read, nor is a t2 sign bit whose mask
    bit is clear."""
    w = np.asarray(w).astype(np.uint32).astype(np.int64)
    P = w.shape[0]
    pw = PER_WORD[kind]
    field = 32 // pw
    sh = np.arange(pw, dtype=np.int64) * field
    if kind == "t2":
        m = ((w[:, 0::2, None] >> sh) & 1).reshape(P, -1)[:, :C]
        s = ((w[:, 1::2, None] >> sh) & 1).reshape(P, -1)[:, :C]
        return m * (2 * s - 1)
    f = ((w[:, :, None] >> sh) & ((1 << field) - 1)).reshape(P, -1)[:, :C]
    if kind == "bin":
        return 2 * f - 1
    return f - ((f >> (field - 1)) << field)


def spare(kind, C):
    """uint32 (words(kind, C),): the bits of a row's words that belong to no channel."""
    return ~encode(np.full((1, C), 1 if kind in ("bin", "t2") else -1, dtype=np.int64), kind)[0]


# ---- codes and their values ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def codes(kind, bits, pixels, C, seed):
    """Integer codes (pixels, C), read-only: bin +-1, t2 {-1, 0, 1}, i4 / i8 the signed `bits`-bit range with both extreme
    codes (-2^(bits-1), 2^(bits-1) - 1) in every tensor: at its first two places, and wherever the draw puts them."""
    rng = np.random.default_rng(zlib.crc32(repr(("merge", kind, bits, pixels, C, seed)).encode()))
    if kind == "bin":
        k = rng.integers(0, 2, (pixels, C)) * 2 - 1
    elif kind == "t2":
        k = rng.integers(-1, 2, (pixels, C))
    else:
        m = 1 << (bits - 1)
        k = rng.integers(-m, m, (pixels, C))
        flat = k.reshape(-1)
        at = seed % (flat.size - 1)                # not the same place in every input, so the extremes also meet other codes
        flat[at], flat[at + 1] = -m, m - 1
    k = np.ascontiguousarray(k, dtype=np.int64)
    k.setflags(write=False)
    return k


def values(k, kind, bits):
    """The float32 values of codes: code / 2^(bits - 1); bin and t2: the code itself.  Exact."""
    return (np.asarray(k, dtype=np.float64) / (1.0 if kind in ("bin", "t2") else float(1 << (bits - 1)))).astype(F32)


def to_codes(v, kind, bits):
    """The inverse of values() (the values must be on the grid)."""
    k = np.asarray(v, dtype=np.float64) * (1.0 if kind in ("bin", "t2") else float(1 << (bits - 1)))
    assert np.array_equal(k, np.rint(k))
    return k.astype(np.int64)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def ref_f32(op, xs, partials=None):
    """Keras' chain in float32: out = x0; out = out o x_i left to right, one rounding per step; avg: the sum chain, then one
    np.float32 division by float32(n); max / min: NaN where either operand is (np.maximum / np.minimum)."""
    xs = [np.asarray(x, dtype=F32) for x in xs]
    assert len(xs) >= 2 and (op != "sub" or len(xs) == 2)
    step = {"add": np.add, "avg": np.add, "sub": np.subtract, "mul": np.multiply, "max": np.maximum, "min": np.minimum}[op]
    out = xs[0]
    with np.errstate(all="ignore"):
        for x in xs[1:]:
            out = step(out, x)
            assert out.dtype == F32
            if partials is not None:
                partials.append(out)
        if op == "avg":
            out = out / F32(len(xs))
            assert out.dtype == F32
    return out


def ref_codes(op, kind, bits, ks):
    """The rules on integer codes: max / min of the codes; mul of +-1 or {-1, 0, 1} codes is their product."""
    assert out_kind(op, kind) == kind and kind != "f32"
    ks = [np.asarray(k, dtype=np.int64) for k in ks]
    if op == "max":
        return np.maximum.reduce(ks)
    if op == "min":
        return np.minimum.reduce(ks)
    return np.multiply.reduce(ks)


# ---- float32 operands --------------------------------------------------------------------------------------------------------
TINY = F32(2.0 ** -126)


def normal_or_zero(a):
    a = np.asarray(a, dtype=F32)
    return bool(np.all((a == 0) | ((np.abs(a) >= TINY) & np.isfinite(a))))


@functools.lru_cache(maxsize=None)
def f32_inputs(op, n, pixels, C, seed=0):
    """n float32 tensors (pixels, C), read-only, magnitudes in 2^-20 .. 2^20 with full 24-bit significands.  The exponents of
    consecutive inputs have opposite signs, so a product of eight stays far inside the normal range; checked: no operand
    and no partial or final result of `op` is subnormal, infinite or NaN."""
    rng = np.random.default_rng(zlib.crc32(repr(("merge-f32", op, n, pixels, C, seed)).encode()))
    xs = []
    for i in range(n):
        e = rng.integers(0, 20, (pixels, C)) * (1 if i % 2 == 0 else -1)
        mant = 1.0 + rng.integers(0, 1 << 23, (pixels, C)) / float(1 << 23)
        x = (rng.choice([-1.0, 1.0], (pixels, C)) * mant * np.exp2(e)).astype(F32)
        assert np.all((np.abs(x) >= F32(2.0 ** -20)) & (np.abs(x) <= F32(2.0 ** 20)))
        x.setflags(write=False)
        xs.append(x)
    partials = []
    out = ref_f32(op, xs, partials)
    assert all(normal_or_zero(p) for p in partials + [out]), (op, n, pixels, C)
    return tuple(xs)


def special_inputs(n=2):
    """The max / min operands beyond the ordinary: +-inf and NaN in either position, both NaN, NaN beside inf, equal values
    and the +-0 pairs (the last four columns), as n tensors (1, 14); inputs beyond the second repeat the first."""
    inf, nan = np.inf, np.nan
    a = [inf, 1.0, -inf, 1.0, nan, 1.0, nan, nan, inf, 2.5, 0.0, -0.0, 0.0, -0.0]
    b = [1.0, inf, 1.0, -inf, 1.0, nan, nan, inf, nan, 2.5, -0.0, 0.0, 0.0, -0.0]
    xs = [np.array([a], dtype=F32), np.array([b], dtype=F32)]
    return xs + [xs[0]] * (n - 2)


ZERO_PAIRS = slice(10, 12)               # the columns of special_inputs whose operands are zeros of opposite sign


def same_f32(got, want, zero_sign_free=None):
    """Bit for bit; a NaN for a NaN whatever its payload; where `zero_sign_free` (a mask or slice) says so a zero for a zero."""
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    if got.shape != want.shape:
        return False
    ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if zero_sign_free is not None:
        free = np.zeros(got.shape, dtype=bool)
        free[..., zero_sign_free] = True
        ok |= free & (got == 0) & (want == 0)
    return bool(np.all(ok))
