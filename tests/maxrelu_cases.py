"""quantized_maxrelu / quantized_leakymaxrelu: a numpy restatement of the contract (include/qnn_abi_maxact.h), the case
list and input points of the reference vectors (golden/ref_maxrelu.npz, written by golden/make_fixtures_maxrelu.py from the
reference's own layers/quantized_ops.py), and the numpy run of a spec the GPU tests compare with.  test_maxrelu_cpu.py
holds the restatement against the vectors."""
import os

import numpy as np

F32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NBS = (2, 3, 4, 8)
ALPHA = F32(0.1)
FNS = ("quantized_maxrelu", "quantized_leakymaxrelu")
# group 1: maxima far from a power of two; group 2: the band where the reference depends on its float32 log
MAXIMA = tuple(F32(mant * 2.0 ** k) for k in (-3, 0, 1, 5) for mant in (1.0625, 1.5, 1.9375))


def _ulps_above(v, n):
    return (np.asarray(v, dtype=F32).view(np.uint32) + np.uint32(n)).view(F32)


AMBIGUOUS = tuple(F32(_ulps_above(F32(2.0 ** k), u)) for k in (-15, 0, 13) for u in range(17))


# ---- the contract ------------------------------------------------------------------------------------------------------
def batch_max(x):
    """M = max over the tensor of max(x, 0) (0 for an empty tensor)."""
    x = np.asarray(x, dtype=F32)
    return F32(np.max(np.maximum(x, F32(0)))) if x.size else F32(0)


def scale_exponent(M):
    """e with P = 2^e the smallest power of two >= M, from M's exponent and mantissa bits; None unless -64 <= e <= 64, i.e. outside
    2^-65 < M <= 2^64 (zero, subnormal, inf and NaN included)."""
    bits = int(np.asarray(M, dtype=F32).view(np.uint32))
    e = (bits >> 23) - 127 + (1 if bits & 0x7FFFFF else 0)
    if bits == 0 or bits >= 0x7F800000 or not -64 <= e <= 64:
        return None
    return e


def leaky(x):
    """L(x): x for x >= 0, float32(0.1) * x (one rounding) for x < 0."""
    x = np.asarray(x, dtype=F32)
    return np.where(x >= 0, x, (ALPHA * x).astype(F32)).astype(F32)


def maxact(x, nb, fn, M=None, shift=0):
    """code = clip(rint(v * (m / P)), lo, m - 1), y = code * (P / m); v = x, lo = 0 (maxrelu) or v = L(x), lo = -m
    (leakymaxrelu).  M: the maximum to scale by (default: that of x; another one for a shard of a batch).  shift: the
    scale's exponent moved by +-1 -- the reference's possible answers inside its ambiguous band, never the contract's."""
    assert fn in FNS
    x = np.asarray(x, dtype=F32)
    e = scale_exponent(batch_max(x) if M is None else M)
    if e is None:
        return np.full(x.shape, np.nan, dtype=F32)
    e += shift
    m = F32(2.0 ** (nb - 1))
    s_in, s_out = F32(2.0 ** (nb - 1 - e)), F32(2.0 ** (e - (nb - 1)))
    v, lo = (x, F32(0)) if fn == "quantized_maxrelu" else (leaky(x), -m)
    with np.errstate(over="ignore", invalid="ignore"):
        code = np.clip(np.rint((v * s_in).astype(F32)), lo, m - F32(1)) + F32(0)      # + 0: a zero code is +0
    return (code * s_out).astype(F32)


def same_bits(a, b):
    """Bit-for-bit equality of two float32 arrays (the sign of a zero included)."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- input points of the reference vectors (arithmetic-free: powers of two, small integers, float32 neighbours) ------------
def around(v):
    """v (float64 points) rounded to float32, with both float32 neighbours of each."""
    c = np.asarray(v, dtype=np.float64).astype(F32)
    return np.concatenate([c, np.nextafter(c, F32(-np.inf)), np.nextafter(c, F32(np.inf))]).astype(F32)


def edge_inputs(nb, M):
    """The points the contract turns on for maximum M at width nb (module docstring of make_fixtures_maxrelu.py); M
    first, every other value <= M."""
    m = 2.0 ** (nb - 1)
    step = 2.0 ** scale_exponent(M) / m
    j = np.arange(-m - 1, m + 1)
    pts = np.concatenate([around((j + 0.5) * step), around(10.0 * (j[j < 0] + 0.5) * step),
                          np.array([0.0, -0.0], dtype=F32),
                          around([(m - 1) * step, -m * step, -10.0 * m * step, 0.0])]).astype(F32)
    return np.concatenate([np.array([M], dtype=F32), pts[pts <= M]]).astype(F32)


def uniform_inputs(M, seed, count=2000):
    u = np.random.default_rng(20261019 + seed).uniform(-1.5, 1.0, count)
    return np.minimum((u * float(M)).astype(F32), F32(M))


def ambiguous_inputs(M, seed):
    x = uniform_inputs(M, 1000 + seed, 127)
    return np.concatenate([np.array([M], dtype=F32), x]).astype(F32)


_npz = {}


def _gold():
    if not _npz:
        _npz.update(np.load(os.path.join(GOLD, "ref_maxrelu.npz")))
    return _npz


def fixture(nb, ci):
    """(x, reference quantized_maxrelu(x, nb), reference quantized_leakymaxrelu(x, nb)) of group 1, case MAXIMA[ci]."""
    d = _gold()
    x = np.concatenate([d["g1_x_nb%d_%d" % (nb, ci)], d["g1_u_%d" % ci]]).astype(F32)
    return x, d["g1_max_nb%d_%d" % (nb, ci)], d["g1_leaky_nb%d_%d" % (nb, ci)]


def fixture_ambiguous(nb, i):
    """The same of group 2, case AMBIGUOUS[i]: recorded answers of the stand-in's float32 log."""
    d = _gold()
    return d["g2_x_%d" % i], d["g2_max_nb%d_%d" % (nb, i)], d["g2_leaky_nb%d_%d" % (nb, i)]


# ---- numpy run of a spec -------------------------------------------------------------------------------------------------
def run_spec(spec, x, float_conv="device", batch_size=None):
    """The oracle's spec interpreter, op by op, with the two activations evaluated by maxact() on the WHOLE batch tensor.
    batch_size: run x in batches of that size, each scaled by its own maxima (what predict(batch_size) computes)."""
    from oracle import qnn_oracle as O
    x = np.asarray(x, dtype=F32)
    if batch_size is not None:
        return np.concatenate([run_spec(spec, x[i:i + batch_size], float_conv) for i in range(0, len(x), batch_size)])
    env = {"input": x}
    cur = x
    O.FLOAT_CONV["order"] = float_conv
    try:
        for i, op in enumerate(spec):
            if op["op"] == "act" and op["fn"] in FNS:
                y = maxact(env[op["src"]] if "src" in op else cur, op["nb"], op["fn"])
            else:
                one, e = dict(op), dict(env)
                e["__cur"] = cur
                if "src" not in one and one["op"] != "add":
                    one["src"] = "__cur"
                y = O._run_spec([one], x, "exact", "legacy", False, env0=e)
            env[op.get("dst", "t%d" % i)] = cur = y
    finally:
        O.FLOAT_CONV["order"] = "ideal"
    return cur
