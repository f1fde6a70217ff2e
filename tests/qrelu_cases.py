"""quantized_relu / quantized_leakyrelu: a numpy restatement of the two arithmetic contracts (include/qnn_abi.h), the
reference's vectors (golden/ref_qrelu.npz, written by golden/make_fixtures_qrelu.py from the reference's own
layers/quantized_ops.py) and the numpy chains the GPU tests compare with -- built from the oracle's conv, BN, pooling and
spec interpreter plus the activations below.  test_qrelu_cpu.py proves the restatement equal to the vectors bit for bit."""
import os

import numpy as np

from oracle import qnn_oracle as O

F32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NBS = (2, 3, 4, 8)
ALPHA = F32(0.1)
FNS = ("quantized_relu", "quantized_leakyrelu")


def quantized_relu(v, nb):
    """u = v + 1 (the only rounding); code = clamp(rint(u * m) - m, 0, m - 1); value = code / m."""
    v = np.asarray(v, dtype=F32)
    m = F32(2 ** (nb - 1))
    u = (v + F32(1)).astype(F32)
    code = np.clip(np.rint(u * m) - m, F32(0), m - F32(1))
    return (code / m).astype(F32)


def _tanh_clip(w, m):
    """clamp(round_through(w * m), -m, m - 1) / m; round_through = t + (rint(t) - t), which is rint(t) with the zero the
    reference produces (+0 for a small negative t)."""
    t = (w * m).astype(F32)
    rt = (t + (np.rint(t) - t).astype(F32)).astype(F32)
    return (np.clip(rt, -m, m - F32(1)) / m).astype(F32)


def quantized_leakyrelu(v, nb, alpha=0.1):
    """w = v for v >= 0, float32(0.1) * v (one rounding) for v < 0; code = clamp(rint(w * m), -m, m - 1)."""
    assert F32(alpha) == ALPHA
    v = np.asarray(v, dtype=F32)
    m = F32(2 ** (nb - 1))
    w = np.where(v >= 0, v, (ALPHA * v).astype(F32)).astype(F32)
    return _tanh_clip(w, m)


def quantized_leakyrelu_max_form(v, nb):
    """The strip kernels' form of the same function: w = max(v, 0.1f * v) instead of the select."""
    v = np.asarray(v, dtype=F32)
    m = F32(2 ** (nb - 1))
    w = np.maximum(v, (ALPHA * v).astype(F32)).astype(F32)
    return _tanh_clip(w, m)


ACT = {"quantized_relu": quantized_relu, "quantized_leakyrelu": quantized_leakyrelu,
       "quantized_tanh": lambda v, nb: O.quantized_tanh(v, nb)}

_fixture = {}


def fixture(nb):
    """(x, reference quantized_relu(x, nb), reference quantized_leakyrelu(x, nb)) out of ref_qrelu.npz."""
    if not _fixture:
        d = np.load(os.path.join(GOLD, "ref_qrelu.npz"))
        for n in NBS:
            x = np.concatenate([d["x_edges_nb%d" % n], d["x_uniform"]]).astype(F32)
            _fixture[n] = (x, d["relu_nb%d" % n], d["leaky_nb%d" % n])
    return _fixture[nb]


def same_bits(a, b):
    """Bit-for-bit equality of two float32 arrays (the sign of a zero included)."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- numpy chains ----------------------------------------------------------------------------------------------------
def run_spec(spec, x, float_conv="device", return_all=False):
    """The oracle's spec interpreter, op by op, with the two activations it does not know evaluated by ACT."""
    env = {"input": np.asarray(x, dtype=F32)}
    cur = env["input"]
    O.FLOAT_CONV["order"] = float_conv
    try:
        for i, op in enumerate(spec):
            if op["op"] == "act" and op["fn"] in FNS:
                y = ACT[op["fn"]](env[op["src"]] if "src" in op else cur, op["nb"])
            else:
                one, e = dict(op), dict(env)
                e["__cur"] = cur
                if "src" not in one and one["op"] != "add":
                    one["src"] = "__cur"
                y = O._run_spec([one], x, "exact", "legacy", False, env0=e)
            env[op.get("dst", "t%d" % i)] = cur = y
    finally:
        O.FLOAT_CONV["order"] = "ideal"
    return env if return_all else cur


def bn_for(cout, seed, both_signs=True, spread=1.0):
    """BN constants with scales of both signs and shifts that push pre-activations over both clips and zero."""
    rng = np.random.default_rng(seed)
    gamma = rng.uniform(0.5, 1.5, cout).astype(F32)
    if both_signs:
        gamma[1::2] *= F32(-1)
    return {"op": "bn", "gamma": gamma, "beta": np.linspace(-1.6, 1.6, cout).astype(F32) * F32(spread),
            "mean": (rng.standard_normal(cout) * 0.1).astype(F32), "var": rng.uniform(0.8, 1.25, cout).astype(F32),
            "eps": 1e-3}


def conv_op(kind, nb, kh, cin, cout, stride, seed, bias=True):
    rng = np.random.default_rng(seed)
    op = {"op": "conv", "kind": kind, "kernel": rng.uniform(-1.0, 1.0, (kh, kh, cin, cout)).astype(F32),
          "bias": (rng.standard_normal(cout) * 0.05).astype(F32) if bias else None, "strides": (stride, stride),
          "padding": "same"}
    if kind == "quantized":
        op["nb"] = nb
    return op


def grid_values(shape, nb, seed):
    """Random values on the grid k / 2^(nb-1) (nb = 1: +-1; nb = 0: ternary {-1, 0, 1})."""
    rng = np.random.default_rng(seed)
    if nb == 0:
        return rng.integers(-1, 2, shape).astype(F32)
    if nb == 1:
        return (rng.integers(0, 2, shape) * 2 - 1).astype(F32)
    m = 2 ** (nb - 1)
    return (rng.integers(-m, m, shape) / m).astype(F32)


def conv_chain(x, op, bn, fn, nb, pool=1, res=None, post_scale=1.0):
    """conv [+ bias] -> BN -> [(res + v) * post_scale] -> fn -> [2x2 max pool], float32, the reference's op order.
    Returns (pre-activation, output)."""
    st = tuple(op["strides"])
    if op["kind"] == "binary":
        v = O.binary_conv2d_call(x, op["kernel"], op.get("bias"), 1.0, None, st, "same")
    else:
        v = O.quantized_conv2d_call(x, op["kernel"], op.get("bias"), op["nb"], None, st, "same")
    if bn is not None:
        v = O.batchnorm_inference(v, bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"])
    if res is not None:
        v = ((np.asarray(res, dtype=F32) + v).astype(F32) * F32(post_scale)).astype(F32)
    y = ACT[fn](v, nb)
    if pool == 2:
        y = O.maxpool2d(y, 2)
    return v, y


def bn_scaled(bn, conv_var):
    """`bn` with its variance set so that BN outputs of a conv with output variance conv_var spread over about [-2, 2]."""
    b = dict(bn)
    b["var"] = (bn["var"] * F32(conv_var)).astype(F32)
    return b
