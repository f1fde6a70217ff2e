"""Whole net specs for the spec engines (engine.GraphModel, LayerModel, ResidualFusedModel, FusedModel) and the numpy
reference they are held against: tests/test_spec_graph_cpu.py proves the reference and the lists,
tests/test_gpu_spec_graph.py runs the engines.  Plain numpy: neither torch nor the package is imported here.

  reference(spec, x)   the whole op vocabulary of the engines, op by op in float32: the ops the oracle knows go through
                       oracle.qnn_oracle._run_spec one at a time, the others to the restatements the suite already proves
                       (pool_cases, qrelu_cases, maxrelu_cases, the zero-stuffed kernel of conv_dilation_cases)
  HAND                 small specs, one per planner decision
  generate(seed)       random specs over the same vocabulary
  guard(spec, x)       None if every comparison of the case may be bit for bit, else the reason
  categories(spec)     the properties the two lists must keep covering (REQUIRED)

Exactness by construction: images lie on k / 8, every weight is drawn on its own grid (so the layers' quantizers are
the identity) and a low-bit activation sits in front of every later contraction, with only max-pools, flattens, zero
padding and power-of-two-area averages in between.  Every product is then a multiple of one power of two and every sum
of magnitudes stays below 2^24 of them, so each contraction is exact in float32 in any order (guard checks it); what
is behind a contraction (bias, BN, add, scale, clip) is the same float32 op sequence everywhere."""
import numpy as np

from oracle import qnn_oracle as O

import conv_dilation_cases as D
import maxrelu_cases as M
import pool_cases as P
import qrelu_cases as Q

F32 = np.float32
N = 3
POOLS = ("maxpool", "avgpool", "globalmaxpool", "globalavgpool")


# ---- reading a spec -----------------------------------------------------------------------------------------------------
def names_of(spec):
    return [op.get("dst", "t%d" % i) for i, op in enumerate(spec)]


def sources(spec):
    """The tensors every op reads: add -> a, b; a named `src`; else the previous op's output; else the images."""
    names = names_of(spec)
    return [[op["a"], op["b"]] if op["op"] == "add" else
            [op["src"] if "src" in op else names[i - 1] if i > 0 else "input"] for i, op in enumerate(spec)]


def consumers(spec):
    cons = {}
    for i, ss in enumerate(sources(spec)):
        for s in ss:
            cons.setdefault(s, []).append(i)
    return cons


def new_pool(op):
    """A pooling op in Keras' form (a pair `size`, `strides`, `padding`, or global) rather than the size-only one."""
    if op["op"] in ("globalmaxpool", "globalavgpool"):
        return True
    return op["op"] in ("maxpool", "avgpool") and ("strides" in op or "padding" in op or
                                                   not isinstance(op.get("size", 2), (int, np.integer)))


def dilation(op):
    return P.pair(op.get("dilation_rate", (1, 1)))


def weights(op):
    """The weights a contraction multiplies by: the oracle's quantizer of its kind applied to the latent kernel."""
    k = np.asarray(op["kernel"], dtype=F32)
    if op["kind"] == "binary":
        return O.binarize(k, op.get("H", 1.0))
    if op["kind"] == "ternary":
        return O._ternarize(k, op.get("H", 1.0))
    if op["kind"] == "quantized":
        return O.quantize(k, op["nb"])
    return k


# ---- the reference ---------------------------------------------------------------------------------------------------------
def _undilated(op):
    """A conv with dilation_rate as the same op on the zero-stuffed kernel.  quantize(0) = 0, so a quantized kernel is
    stuffed as it is; 0 is neither a binary nor a ternary weight (and would move the ternary cutoff), so those are
    quantized first and contracted as a stock conv."""
    dh, dw = dilation(op)
    one = {k: v for k, v in op.items() if k != "dilation_rate"}
    if op["kind"] == "quantized":
        one["kernel"] = D.stuff(np.asarray(op["kernel"], dtype=F32), dh, dw)
    else:
        one.update(kind="float", kernel=D.stuff(weights(op), dh, dw))
    return one


def reference(spec, x, return_all=False):
    """Interpret `spec` on NHWC float32 `x`: the last tensor, or the dict of all of them."""
    x = np.asarray(x, dtype=F32)
    env, cur = {"input": x}, x
    O.FLOAT_CONV["order"] = "device"
    try:
        for i, op in enumerate(spec):
            kind = op["op"]
            src = env[op["src"]] if "src" in op else cur
            if kind in ("globalmaxpool", "globalavgpool"):
                y = P.global_ref(src, kind[6:9])
            elif kind in ("maxpool", "avgpool") and new_pool(op):
                y = P.pool2d_ref(src, kind[:3], op.get("size", 2 if kind == "maxpool" else 8), op.get("strides"),
                                 str(op.get("padding", "valid")).lower())
            elif kind == "act" and op["fn"] in Q.FNS:
                if op["fn"] == "quantized_leakyrelu":
                    assert F32(op.get("alpha", Q.ALPHA)) == Q.ALPHA
                y = Q.ACT[op["fn"]](src, op["nb"])
            elif kind == "act" and op["fn"] in M.FNS:
                assert F32(op.get("alpha", M.ALPHA)) == M.ALPHA
                y = M.maxact(src, op["nb"], op["fn"])
            else:
                one = _undilated(op) if kind == "conv" and dilation(op) != (1, 1) else dict(op)
                e = dict(env)
                e["__cur"] = cur
                if "src" not in one and kind != "add":
                    one["src"] = "__cur"
                y = O._run_spec([one], x, "exact", "legacy", False, env0=e)
            env[op.get("dst", "t%d" % i)] = cur = np.asarray(y, dtype=F32)
    finally:
        O.FLOAT_CONV["order"] = "ideal"
    return env if return_all else cur


# ---- the guard -------------------------------------------------------------------------------------------------------------
def _codes(v, what):
    """(integer codes, a) with v = codes * 2^-a exactly, for the smallest such a <= 24."""
    v64 = np.asarray(v, dtype=np.float64)
    for a in range(25):
        k = v64 * float(2 ** a)
        if np.array_equal(k, np.rint(k)):
            return np.rint(k).astype(np.int64), a
    raise ValueError("%s is not dyadic to 2^-24" % what)


def _contract(x, w, op):
    """Integer contraction of codes: conv (the stuffed window for a dilated one) or matrix product."""
    if op["op"] == "dense":
        return x.dot(w)
    dh, dw = dilation(op)
    return O.int_conv2d(x, D.stuff(w, dh, dw), tuple(op.get("strides", (1, 1))), op.get("padding", "same"))


def guard(spec, x):
    """None if the case is exact by construction, else why not.  Every contraction: operands dyadic, the float64 result
    equal to its float32 rounding, and the sum of the products' magnitudes below 2^24 units, which makes every partial
    sum in every order exact as well.  ternary_tanh and the two batch-maximum activations: no value changes code when
    the batch statistic moves by one float32 ulp either way (the engines reduce in float32, the reference in float64)."""
    env = reference(spec, x, return_all=True)
    for i, (op, ss) in enumerate(zip(spec, sources(spec))):
        src = env[ss[0]]
        if op["op"] in ("conv", "dense"):
            try:
                xc, a = _codes(src, "input of op %d" % i)
                wc, b = _codes(weights(op), "weights of op %d" % i)
            except ValueError as e:
                return str(e)
            s64 = _contract(xc, wc, op).astype(np.float64) * 2.0 ** -(a + b)
            if not np.array_equal(s64.astype(F32).astype(np.float64), s64):
                return "op %d: the float64 contraction is not a float32 value" % i
            if _contract(np.abs(xc), np.abs(wc), op).max(initial=0) >= 2 ** 24:
                return "op %d: partial sums may pass 2^24 units" % i
        elif op["op"] == "act" and op["fn"] == "ternary_tanh":
            t = np.clip(src, F32(-1), F32(1))
            mean = F32(np.mean(np.abs(t), dtype=np.float64))
            lo = np.nextafter(F32(0.7) * np.nextafter(mean, F32(-np.inf)), F32(-np.inf))
            hi = np.nextafter(F32(0.7) * np.nextafter(mean, F32(np.inf)), F32(np.inf))
            if np.any((np.abs(t) >= lo) & (np.abs(t) <= hi)):
                return "op %d: a value within one ulp of the ternary cutoff" % i
        elif op["op"] == "act" and op["fn"] in M.FNS:
            mx = M.batch_max(src)
            for m2 in (np.nextafter(mx, F32(-np.inf)), np.nextafter(mx, F32(np.inf))):
                if not M.same_bits(M.maxact(src, op["nb"], op["fn"], M=m2), env[names_of(spec)[i]]):
                    return "op %d: the batch maximum is within one ulp of a power of two or a rounding tie" % i
    return None


# ---- building specs --------------------------------------------------------------------------------------------------------
def _kernel(rng, kind, nb, shape):
    """Weights on the grid of their kind: the layer's quantizer leaves them as they are."""
    if kind == "binary":
        return (rng.integers(0, 2, shape) * 2 - 1).astype(F32)
    if kind == "ternary":
        k = rng.integers(-1, 2, shape).astype(F32)
        k.flat[:2] = (1, -1)                     # never all zero: the cutoff 0.7 mean|w| stays inside (0, 1)
        return k
    if kind == "quantized":
        m = 2 ** (nb - 1)
        return (rng.integers(-m, m, shape) / float(m)).astype(F32)
    return (rng.integers(-16, 17, shape) / 16.0).astype(F32)


_WVAR = {"binary": 1.0, "ternary": 0.67, "quantized": 0.33, "float": 0.33}


class Net:
    """A spec under construction: every method appends one op, reads the previous op's tensor unless `src` names another,
    and returns the name of what it wrote.  An op that reads its predecessor carries no `src`, as the chain builder of
    nets.py leaves it (FusedModel takes nothing else)."""

    def __init__(self, seed, hw=(8, 8), cin=3):
        self.rng = np.random.default_rng(seed)
        self.spec, self.shape, self.cur, self.hw, self.cin = [], {"input": (hw[0], hw[1], cin)}, "input", hw, cin

    def images(self):
        h, w = self.hw
        return (np.random.default_rng(77).integers(0, 9, (N, h, w, self.cin)) / 8.0).astype(F32)

    def _put(self, op, src, shape, dst=None):
        prev = names_of(self.spec)[-1] if self.spec else "input"
        src = self.cur if src is None else src
        if src != prev:
            op["src"] = src
        if dst is not None:
            op["dst"] = dst
        self.spec.append(op)
        name = names_of(self.spec)[-1]
        assert name not in self.shape, name
        self.shape[name] = shape
        self.cur = name
        return name

    def conv(self, cout, kind="quantized", nb=4, k=3, s=1, pad="same", bias=False, src=None, dil=None, dst=None):
        h, w, cin = self.shape[self.cur if src is None else src]
        kh, kw = P.pair(k)
        op = {"op": "conv", "kind": kind, "kernel": _kernel(self.rng, kind, nb, (kh, kw, cin, cout)),
              "bias": (self.rng.standard_normal(cout) * 0.05).astype(F32) if bias else None, "strides": (s, s),
              "padding": pad}
        if kind == "quantized":
            op["nb"] = nb
        dh, dw = (1, 1) if dil is None else P.pair(dil)
        if dil is not None:
            op["dilation_rate"] = (dh, dw)
        ho, wo = (P.axis(n, D.effective(kk, d), s, pad == "same")[0] for n, kk, d in ((h, kh, dh), (w, kw, dw)))
        self.fan = kh * kw * cin * _WVAR[kind]
        return self._put(op, src, (ho, wo, cout), dst)

    def dense(self, units, kind="quantized", nb=4, bias=False, src=None, dst=None):
        (k,) = self.shape[self.cur if src is None else src]
        op = {"op": "dense", "kind": kind, "kernel": _kernel(self.rng, kind, nb, (k, units)),
              "bias": (self.rng.standard_normal(units) * 0.05).astype(F32) if bias else None}
        if kind == "quantized":
            op["nb"] = nb
        self.fan = k * _WVAR[kind]
        return self._put(op, src, (units,), dst)

    def bn(self, src=None, dst=None):
        """Random constants with scales of both signs, as tests/test_gpu_random.py draws them."""
        shape = self.shape[self.cur if src is None else src]
        c, rng, var = shape[-1], self.rng, max(1.0, self.fan * 0.3)
        op = dict(op="bn", eps=1e-3, gamma=(rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(F32),
                  beta=(rng.standard_normal(c) * 0.5).astype(F32), mean=(rng.standard_normal(c) * 0.1 * np.sqrt(var)).astype(F32),
                  var=(var * rng.uniform(0.8, 1.25, c)).astype(F32))
        return self._put(op, src, shape, dst)

    def act(self, fn="quantized_tanh", nb=4, src=None, dst=None, alpha=None):
        op = {"op": "act", "fn": fn}
        if fn.startswith("quantized"):
            op["nb"] = nb
        if alpha is not None:
            op["alpha"] = alpha
        return self._put(op, src, self.shape[self.cur if src is None else src], dst)

    def add(self, a, b, dst=None):
        assert self.shape[a] == self.shape[b], (self.shape[a], self.shape[b])
        op = {"op": "add", "a": a, "b": b}
        if dst is not None:
            op["dst"] = dst
        self.spec.append(op)
        name = names_of(self.spec)[-1]
        self.shape[name] = self.shape[a]
        self.cur = name
        return name

    def scale(self, value, src=None):
        return self._put({"op": "scale", "value": value}, src, self.shape[self.cur if src is None else src])

    def pool(self, kind, size=None, strides=None, padding=None, src=None, dst=None):
        h, w, c = self.shape[self.cur if src is None else src]
        op = {"op": kind}
        if kind.startswith("global"):
            return self._put(op, src, (c,), dst)
        for key, v in (("size", size), ("strides", strides), ("padding", padding)):
            if v is not None:
                op[key] = v
        sz = op.get("size", 2 if kind == "maxpool" else 8)
        if new_pool(op):
            (ph, pw), same = P.pair(sz), padding == "same"
            sh, sw = (ph, pw) if strides is None else P.pair(strides)
            shape = (P.axis(h, ph, sh, same)[0], P.axis(w, pw, sw, same)[0], c)
        else:
            shape = (h // sz, w // sz, c)
        assert shape[0] > 0 and shape[1] > 0, shape
        return self._put(op, src, shape, dst)

    def zeropad(self, pad, src=None):
        h, w, c = self.shape[self.cur if src is None else src]
        return self._put({"op": "zeropad", "pad": pad}, src, (h + 2 * pad, w + 2 * pad, c))

    def flatten(self, src=None, dst=None):
        return self._put({"op": "flatten"}, src, (int(np.prod(self.shape[self.cur if src is None else src])),), dst)

    def softmax(self, src=None):
        return self._put({"op": "softmax"}, src, self.shape[self.cur if src is None else src])

    # a few groups the cases below repeat
    def group(self, cout, kind="quantized", nb=4, fn="quantized_tanh", abits=4, **kw):
        self.conv(cout, kind, nb, **kw)
        self.bn()
        return self.act(fn, abits)

    def classifier(self, kind="quantized", nb=4):
        self.flatten()
        return self.dense(10, kind, nb, bias=True)


ACT_OF = {"bin": ("binary_tanh", 1), "q2": ("quantized_tanh", 2), "q3": ("quantized_tanh", 3), "q4": ("quantized_tanh", 4),
          "q8": ("quantized_tanh", 8), "relu4": ("quantized_relu", 4), "leaky4": ("quantized_leakyrelu", 4),
          "tern": ("ternary_tanh", 1), "relu8": ("quantized_relu", 8), "leaky2": ("quantized_leakyrelu", 2)}
WEIGHT_OF = {"bin": ("binary", 1), "tern": ("ternary", 1), "q2": ("quantized", 2), "q3": ("quantized", 3),
             "q4": ("quantized", 4), "q8": ("quantized", 8)}

# FusedModel on the case: it runs; FusedModel._group refuses the spec; _group takes the chain and the constructor refuses
RUNS, NO_GROUP, NO_CTOR = "runs", "refuses in _group", "refuses in the constructor"

HAND = []


def _case(name, net, fused, exact=True, **expect):
    """expect: what the GPU file asserts about the plan (see test_gpu_spec_graph.py)."""
    assert name not in [c["name"] for c in HAND], name
    HAND.append(dict(name=name, spec=net.spec, x=net.images(), fused=fused, exact=exact, **expect))


def _seed(name):
    import zlib
    return zlib.crc32(name.encode())


# -- flatten in front of a wider dense
# ResidualFusedModel._act_out_store: the dense behind the flatten joins the activation's store, widened to whole words
for _a, _d in (("q4", "q8"), ("bin", "q4"), ("bin", "bin")):
    for _c in (8, 32, 12, 24):
        for _pool in (False, True):
            _n = "flatten_%s_dense_%s_c%d%s" % (_a, _d, _c, "_pool" if _pool else "")
            net = Net(_seed(_n), hw=(4, 4))
            net.group(_c, *WEIGHT_OF["q4"], *ACT_OF[_a])
            if _pool:
                net.pool("maxpool", (2, 2), (2, 2), "valid")
            net.classifier(*WEIGHT_OF[_d])
            _case(_n, net, NO_GROUP if _pool else RUNS, flatten_dense=True)

# -- one activation, two contractions with different weight stores
# _act_out_store: joins of a binary and an 8-bit conv -> one int8 tensor; _fusable_before: both operands conv -> bn
net = Net(1, hw=(8, 8))
a0 = net.group(16, "quantized", 4, "binary_tanh", 1)
net.conv(16, "binary", 1, src=a0)
b1 = net.bn()
net.conv(16, "quantized", 8, src=a0)
b2 = net.bn()
net.add(b1, b2)
net.act("quantized_tanh", 4)
net.classifier()
_case("two_stores_bin_and_q8", net, NO_GROUP)

# _act_out_store: a contraction and a new-form average pool read the same codes
net = Net(2, hw=(8, 8))
a0 = net.group(16)
p = net.pool("avgpool", (2, 2), (2, 2), "valid", src=a0)
net.conv(16, s=2, src=a0)
b = net.bn()
net.add(p, b)
net.scale(0.5)
net.act()
net.classifier()
_case("conv_and_new_avgpool_read_one_act", net, NO_GROUP)


# -- residual merges
def _block(name, a="q4", w="q4", c=16, main_as="b", scale=0.5, merge=None, short="identity", hw=(8, 8), head="tail",
           dil=None, s=1, c2=None, short_k=1, extra=None):
    """stem -> a0; main path conv -> bn -> act -> conv -> bn; shortcut of kind `short`; add; [scale]; merge act; head."""
    net = Net(_seed(name), hw=hw)
    (wk, wn), (fn, ab) = WEIGHT_OF[w], ACT_OF[a]
    c2 = c if c2 is None else c2
    a0 = net.group(c, wk, wn, fn, ab, dst="a0")
    net.conv(c2, wk, wn, s=s, src=a0)
    net.bn()
    net.act(fn, ab)
    net.conv(c2, wk, wn, dil=dil)
    b2 = net.bn(dst="b2")
    if short == "identity":
        sh = a0
    elif short == "conv":                                    # the float32 output of a projection conv
        sh = net.conv(c2, wk, wn, k=short_k, s=s, src=a0, dst="proj")
    elif short == "bn":                                      # ... with a BN behind it
        net.conv(c2, wk, wn, k=1, s=s, src=a0)
        sh = net.bn(dst="proj_bn")
    if extra == "proj_read_twice":                           # the projection also feeds a second add
        net.act(fn, ab, src=sh, dst="side")
    merged = net.add(b2, sh) if main_as == "a" else net.add(sh, b2)
    if scale is not None:
        net.scale(scale)
    mf, mb = ACT_OF[merge or a]
    am = net.act(mf, mb, dst="am")
    if extra == "proj_read_twice":
        net.add("side", am)
        net.act(fn, ab)
    if head == "tail":
        h, w_, _ = net.shape[net.cur]
        net.pool("avgpool", 1 << (min(h, w_).bit_length() - 1))      # a power-of-two area: the averages stay dyadic
        net.flatten()
        net.dense(10, wk, wn)
    else:
        net.classifier(wk, wn)
    return net


# ResidualFusedModel._fusable_before: the main path as operand b (the builders' order) and as operand a
_case("merge_main_is_b", _block("merge_main_is_b"), NO_GROUP)
_case("merge_main_is_a", _block("merge_main_is_a", main_as="a"), NO_GROUP)
# _fusable_before: post = 1.0 without a scale op; a scale that is not the builders' 0.5
_case("merge_no_scale", _block("merge_no_scale", scale=None), NO_GROUP)
_case("merge_scale_quarter", _block("merge_scale_quarter", scale=0.25, main_as="a"), NO_GROUP)
# _plan / _conv_call: the merge activation in the epilogue, every function and width
for _m in ("q2", "q4", "q8", "bin", "relu4", "leaky4"):
    _case("merge_act_%s" % _m, _block("merge_act_%s" % _m, merge=_m, head="flat"), NO_GROUP)
# _conv_call: the shortcut operand as packed int4 / binary / int8 codes, ternary planes, float32 BN and conv outputs
_case("short_i4_strip", _block("short_i4_strip", merge="relu4"), NO_GROUP, kernels=["strip_i4_c16"])
_case("short_bin", _block("short_bin", a="bin", w="bin"), NO_GROUP)
_case("short_i8", _block("short_i8", a="q8", w="q8", head="flat"), NO_GROUP)
_case("short_ternary_planes", _block("short_ternary_planes", a="tern", w="tern"), NO_GROUP)
_case("short_bn_f32", _block("short_bn_f32", short="bn", hw=(9, 7)), NO_GROUP)
_case("short_conv_f32", _block("short_conv_f32", short="conv", hw=(9, 7)), NO_GROUP)
# _fusable_before finds nothing: add of two activations, add of a tensor with itself
net = Net(3)
a0 = net.group(8)
a1 = net.group(8)
net.add(a0, a1)
net.act()
net.classifier()
_case("add_of_two_acts", net, NO_GROUP)
net = Net(4)
net.group(8)
net.conv(8)
b = net.bn()
net.add(b, b)
net.scale(0.5)
net.act()
net.classifier()
_case("add_of_a_tensor_with_itself", net, NO_GROUP)
# _conv_bn_of: a bn read by the act and by an add must stay a tensor
net = Net(5)
a0 = net.group(16)
net.conv(16)
b1 = net.bn()
net.act()
net.conv(16)
b2 = net.bn()
net.add(b1, b2)
net.act()
net.classifier()
_case("bn_read_by_act_and_add", net, NO_GROUP)

# -- the in-launch projection (ResidualFusedModel._projection_of)
_PROJ = dict(c=16, c2=32, s=2, short="conv", hw=(8, 8))
_case("projection_eligible", _block("projection_eligible", **_PROJ), NO_GROUP, projection="fused")
_case("projection_read_twice", _block("projection_read_twice", extra="proj_read_twice", head="flat", **_PROJ), NO_GROUP,
      projection="pw")
_case("projection_3bit_act", _block("projection_3bit_act", merge="q3", **_PROJ), NO_GROUP, projection="pw")
_case("projection_relu_merge", _block("projection_relu_merge", merge="relu4", **_PROJ), NO_GROUP, projection="pw")
_case("projection_3x3", _block("projection_3x3", short_k=3, **_PROJ), NO_GROUP, projection="other")
_case("projection_dilated_main", _block("projection_dilated_main", dil=2, **_PROJ), NO_GROUP, projection="pw")
# _conv_call: one dilated conv inside a residual block
_case("dilated_in_residual", _block("dilated_in_residual", dil=(2, 2), hw=(9, 7)), NO_GROUP)

# -- pools
# _act_out_store looks through a new-form max-pool: the codes stay packed for the conv behind it
for _a, _w in (("bin", "bin"), ("q4", "q4"), ("q8", "q8")):
    net = Net(_seed("pool" + _a), hw=(9, 7))
    net.group(16, *WEIGHT_OF[_w], *ACT_OF[_a])
    net.pool("maxpool", (3, 3), (2, 2), "same")
    net.group(16, *WEIGHT_OF[_w], *ACT_OF[_a])
    net.classifier(*WEIGHT_OF[_w])
    _case("new_maxpool_%s" % _a, net, NO_GROUP, packed_pools=["pool_max_" + {"bin": "bin", "q4": "i4", "q8": "i8"}[_a]])
net = Net(6, hw=(9, 7))
net.group(8)
net.pool("maxpool", (2, 2), (1, 1), "same")
net.pool("maxpool", (3, 2), (2, 2), "valid")
net.group(8)
net.classifier()
_case("two_pools_in_a_row", net, NO_GROUP, packed_pools=["pool_max_i4", "pool_max_i4"])
net = Net(7)
net.group(16, "quantized", 4, "binary_tanh", 1)
net.pool("globalmaxpool")
net.dense(10, "binary", 1, bias=True)
_case("global_maxpool_dense", net, NO_GROUP)
net = Net(8)
net.group(8)
net.pool("avgpool", (2, 2), (2, 2), "valid")
net.classifier()
_case("new_avgpool_dense", net, NO_GROUP)
# _compute: an old-form pool on packed codes goes through float32 (and back for the merge's shortcut)
net = Net(9)
net.group(16)
a0 = net.pool("maxpool", 2)
net.group(16)
net.conv(16)
b = net.bn()
net.add(a0, b)
net.scale(0.5)
net.act()
net.classifier()
_case("old_pool_in_residual", net, NO_GROUP)
# FusedModel._group: a size-2 pool with strides (1, 1) is not the epilogue pool
net = Net(10)
net.group(8)
net.pool("maxpool", 2, (1, 1))
net.group(8)
net.classifier()
_case("chain_pool_with_unit_strides", net, NO_GROUP, packed_pools=["pool_max_i4"])
net = Net(11)
net.group(8)
net.pool("maxpool", 2)
net.group(8, pad="valid")
net.pool("maxpool", 2)
net.classifier()
_case("chain_old_pools", net, RUNS)

# -- classifier tails (_SpecGraph.tail / tail_from)
for _n, _sm in (("tail", False), ("tail_softmax", True)):
    net = Net(_seed(_n))
    net.group(16)
    net.pool("avgpool", 8)
    net.flatten()
    net.dense(10)
    if _sm:
        net.softmax()
    _case(_n, net, NO_GROUP, tail="tail_avg_dense_softmax" if _sm else "tail_avg_dense")
net = Net(12)
net.group(16)
p = net.pool("avgpool", 4)
net.flatten()
d = net.dense(10)
net.flatten(src=p)
d2 = net.dense(10)
net.add(d, d2)
_case("tail_avgpool_read_twice", net, NO_GROUP, tail=None)
net = Net(13)
net.group(16)
net.pool("avgpool", (8, 8), (8, 8), "valid")
net.flatten()
net.dense(10)
_case("tail_new_form_avgpool", net, NO_GROUP, tail="dense_f32")
net = Net(14)
net.group(16)
net.pool("avgpool", 8)
net.flatten()
net.dense(10)
net.bn()
_case("tail_dense_not_last", net, NO_GROUP, tail="dense_f32")

# -- other glue
net = Net(15)
net.group(8)
net.zeropad(1)
net.group(8, pad="valid")
net.classifier()
_case("zeropad_valid_conv", net, NO_GROUP)
net = Net(16)                                                # _conv_call: a stock float conv reads unpacked codes
net.group(8)
net.group(8, "float", 0)
net.classifier()
_case("float_conv_mid_network", net, NO_CTOR, float_layers=True)
net = Net(17)
net.conv(8, bias=True)
net.act()
net.classifier()
_case("conv_without_bn", net, RUNS)
net = Net(18)
net.group(8)
net.conv(8, bias=True)
_case("conv_is_last", net, RUNS)
net = Net(19)
net.group(8)
net.conv(8)
net.bn()
_case("bn_is_last", net, RUNS)
net = Net(20)                                                # the demand-driven engines never compute t3
a0 = net.group(8)
net.pool("maxpool", (2, 2), (2, 2), "valid")
net.flatten(src=a0)
net.dense(10)
_case("dead_op", net, NO_GROUP)
# ResidualFusedModel._plan: LeakyReLU(0.3) is fused into the float-activation kernels, 0.1 is not
for _alpha in (0.3, 0.1):
    net = Net(21)
    net.conv(8, "float", 0, bias=True)
    net.bn()
    a0 = net.act("leaky_relu", alpha=_alpha)
    net.conv(8, "float", 0)
    b = net.bn()
    net.add(a0, b)
    net.act("leaky_relu", alpha=_alpha)
    net.classifier("float", 0)
    _case("leaky_relu_%s" % str(_alpha).replace(".", "_"), net, NO_GROUP, exact=False, float_layers=True)
# _plan: ternary_tanh read only by ternary contractions through a max-pool (T2 planes), and by a quantized conv as well
net = Net(22)
net.group(8, "ternary", 1, "ternary_tanh", 1)
net.pool("maxpool", 2)
net.group(8, "ternary", 1, "ternary_tanh", 1)
net.classifier("ternary", 1)
_case("ternary_through_maxpool", net, NO_CTOR)
net = Net(23)
a0 = net.group(8, "ternary", 1, "ternary_tanh", 1)
net.conv(8, "ternary", 1, src=a0)
b1 = net.bn()
net.conv(8, "quantized", 4, src=a0)
b2 = net.bn()
net.add(b1, b2)
net.act("ternary_tanh")
net.classifier("ternary", 1)
_case("ternary_read_by_a_quantized_conv", net, NO_GROUP)
# GraphModel only: the batch-maximum activations (the packed engines refuse them)
net = Net(24)
net.group(8, fn="quantized_maxrelu", abits=4)
net.group(8, fn="quantized_leakymaxrelu", abits=3)
net.classifier()
_case("max_activations", net, NO_CTOR, max_acts=True)

net = Net(25)
net.group(8, fn="quantized_leakymaxrelu", abits=4)
net.pool("maxpool", (2, 2), (2, 2), "same")
net.group(8, fn="quantized_maxrelu", abits=2)
net.classifier()
_case("max_activations_and_a_pool", net, NO_GROUP, max_acts=True)
# _act_out_store: a global average reads the codes; the float32 means go to the dense
for _n, _sm in (("global_avgpool_dense", False), ("global_avgpool_dense_softmax", True)):
    net = Net(_seed(_n))
    net.group(16, "binary", 1, "binary_tanh", 1)
    net.pool("globalavgpool")
    net.dense(10, "binary", 1)
    if _sm:
        net.softmax()
    _case(_n, net, NO_GROUP)
# each shortcut kind and the eligible projection a second time, at other sizes
_case("short_bin_main_a", _block("short_bin_main_a", a="bin", w="bin", c=32, main_as="a", scale=None, head="flat"), NO_GROUP)
_case("short_i8_c32", _block("short_i8_c32", a="q8", w="q8", c=32, hw=(9, 7)), NO_GROUP)
_case("short_ternary_main_a", _block("short_ternary_main_a", a="tern", w="tern", c=8, main_as="a", head="flat"), NO_GROUP)
_case("short_bn_f32_strided", _block("short_bn_f32_strided", short="bn", s=2, c2=32), NO_GROUP)
_case("projection_eligible_c64", _block("projection_eligible_c64", c=32, c2=64, s=2, short="conv", hw=(8, 8)), NO_GROUP,
      projection="fused")

PIPELINED = ("merge_main_is_b", "two_pools_in_a_row", "flatten_q4_dense_q8_c12")


# ---- the generator ---------------------------------------------------------------------------------------------------------
SEEDS = range(48)
CHANNELS = (8, 12, 16, 24, 32, 64)


def generate(seed):
    """(spec, images) of a random network: a stem, 2 to 5 blocks out of {plain group, residual block with identity,
    projection or float shortcut, pool, zeropad + valid conv}, and a head out of {flatten -> dense, tail, global pool ->
    dense}; at most 6 contractions."""
    rng = np.random.default_rng(90000 + seed)
    net = Net(50000 + seed, hw=(8, 8) if rng.random() < 0.5 else (9, 7))
    pick = lambda seq: seq[int(rng.integers(len(seq)))]      # noqa: E731
    int4 = rng.random() < 0.5                                # a 16 / 32 / 64-channel int4 network: strips, folds, projections
    wkeys = ("q4",) if int4 else ("bin", "tern", "q2", "q3", "q4", "q8")
    akeys = ("q4", "q4", "relu4", "leaky4") if int4 else ("bin", "q2", "q3", "q4", "q8", "relu4", "relu8", "leaky2", "tern")
    chans = (16, 32, 64) if int4 else CHANNELS
    contractions = [1]

    def w():
        return WEIGHT_OF[pick(wkeys)]

    def a():
        return ACT_OF[pick(akeys)]

    def conv(cout, **kw):
        contractions[0] += 1
        return net.conv(cout, *w(), bias=bool(rng.random() < 0.5), **kw)

    c = pick(chans[:4] if not int4 else (16, 32))
    net.conv(c, *w(), bias=bool(rng.random() < 0.5))
    if rng.random() < 0.8:
        net.bn()
    cur = net.act(*a())
    for _ in range(int(rng.integers(2, 6))):
        h, w_, c = net.shape[cur]
        block = pick(("group", "group", "identity", "projection", "float_shortcut", "pool", "zeropad"))
        room = 6 - 1 - contractions[0]                       # (the head's dense is one)
        if block == "pool" and min(h, w_) >= 4:
            if rng.random() < 0.3:
                cur = net.pool("maxpool", 2)
            else:
                cur = net.pool("maxpool", pick(((2, 2), (3, 3), (2, 3))), pick(((2, 2), (1, 1), (2, 1))), pick(("same", "valid")))
        elif block == "zeropad" and room >= 1:
            net.zeropad(1)
            conv(pick(chans), pad="valid")
            net.bn()
            cur = net.act(*a())
        elif block in ("identity", "float_shortcut") and room >= 2 + (block == "float_shortcut"):
            fn_ab = a()
            conv(c, src=cur)
            net.bn()
            net.act(*fn_ab)
            conv(c)
            main = net.bn()
            short = cur
            if block == "float_shortcut":
                conv(c, k=1, src=cur)
                short = net.bn() if rng.random() < 0.5 else net.cur
            net.add(short, main) if rng.random() < 0.7 else net.add(main, short)
            sc = pick((0.5, 0.5, None, 0.25))
            if sc is not None:
                net.scale(sc)
            cur = net.act(*(fn_ab if rng.random() < 0.7 else a()))
        elif block == "projection" and room >= 3 and min(h, w_) >= 4:
            c2 = 2 * c if 2 * c <= 64 and rng.random() < 0.8 else c
            fn_ab = a()
            conv(c2, s=2, src=cur)
            net.bn()
            net.act(*fn_ab)
            conv(c2)
            main = net.bn()
            short = conv(c2, k=1, s=2, src=cur)
            net.add(short, main)
            net.scale(0.5)
            cur = net.act(*fn_ab)
        elif room >= 1:
            conv(pick(chans), s=2 if (rng.random() < 0.25 and min(h, w_) >= 4) else 1)
            if rng.random() < 0.8:
                net.bn()
            cur = net.act(*a())
    h, w_, c = net.shape[cur]
    head = pick(("flat", "tail", "global"))
    if head == "flat":
        net.flatten()
    elif head == "tail":
        s = 8 if min(h, w_) >= 8 else 4 if min(h, w_) >= 4 else 2 if min(h, w_) >= 2 else 1
        net.pool("avgpool", s)
        net.flatten()
    else:
        pow2 = (h * w_) & (h * w_ - 1) == 0                  # a global average stays dyadic over a power-of-two image only
        net.pool("globalavgpool" if pow2 and rng.random() < 0.5 else "globalmaxpool")
    net.dense(10, *w(), bias=bool(head != "tail" and rng.random() < 0.5))
    if rng.random() < 0.3:
        net.softmax()
    x = (rng.integers(0, 9, (N, net.hw[0], net.hw[1], 3)) / 8.0).astype(F32)
    return net.spec, x


# ---- what the lists must cover ---------------------------------------------------------------------------------------------
def _wclass(op):
    """The packed store a contraction's weights ask for: bin, i4, i8, or f32."""
    if op["kind"] == "binary":
        return "bin"
    if op["kind"] == "ternary":
        return "i4"
    if op["kind"] == "quantized" and op["nb"] <= 8:
        return "i4" if op["nb"] <= 4 else "i8"
    return "f32"


def chain(spec):
    """True if the spec is the chain FusedModel._group takes: [conv | dense] [bn] [act] [old-form 2 x 2 max-pool behind a
    conv] [softmax] groups with flattens anywhere, every op reading its predecessor, no conv behind a dense, square strides."""
    i, n, seen_dense = 0, len(spec), False
    while i < n:
        op = spec[i]
        if "src" in op and i > 0:
            return False
        if op["op"] == "flatten":
            i += 1
            continue
        if op["op"] not in ("conv", "dense"):
            return False
        if op["op"] == "conv" and (seen_dense or len(set(op.get("strides", (1, 1)))) != 1):
            return False
        seen_dense |= op["op"] == "dense"
        first = op["op"]
        i += 1
        for kind in ("bn", "act", "maxpool", "softmax"):
            if i < n and spec[i]["op"] == kind:
                if kind == "maxpool" and (new_pool(spec[i]) or spec[i].get("size", 2) != 2 or first != "conv"):
                    return False
                i += 1
    return True


def _projection(spec, names, cons, prod, main, short, ai):
    """"eligible" / "near miss" / None for the merge of conv `main` with shortcut tensor `short` in front of `act`: what
    ResidualFusedModel._projection_of decides, restated.  A near miss is a strides-2 conv as the shortcut that fails one
    condition."""
    pi = prod.get(short)
    if pi is None or spec[pi]["op"] != "conv" or tuple(spec[pi].get("strides", (1, 1))) != (2, 2):
        return None
    po, mo, act = spec[pi], spec[main], spec[ai]
    pk, mk = po["kernel"].shape, mo["kernel"].shape
    ok = (len(cons.get(short, [])) == 1 and po["kind"] == "quantized" and po.get("nb") == 4 and mo["kind"] == "quantized" and
          mo.get("nb") == 4 and tuple(pk[:2]) == (1, 1) and tuple(mk[:2]) == (3, 3) and
          tuple(mo.get("strides", (1, 1))) == (1, 1) and mo.get("padding", "same") == "same" and dilation(po) == (1, 1) and
          dilation(mo) == (1, 1) and mk[2] == mk[3] and mk[3] in (32, 64) and pk[3] == mk[3] and 2 * pk[2] == mk[2] and
          act["fn"] == "quantized_tanh" and act["nb"] == 4)
    if ok:                                                   # ... and every reader of the activation takes int4 codes
        todo = [names[ai]]
        while todo:
            for ci in cons.get(todo.pop(), []):
                o = spec[ci]
                if o["op"] in ("conv", "dense"):
                    ok &= _wclass(o) == "i4"
                elif o["op"] in ("maxpool", "globalmaxpool", "flatten") and (o["op"] == "flatten" or new_pool(o)):
                    todo.append(names[ci])
                elif o["op"] not in ("add", "avgpool", "globalavgpool"):
                    ok = False
    return "eligible" if ok else "near miss"


def categories(spec):
    names, srcs, cons = names_of(spec), sources(spec), consumers(spec)
    prod = {n: i for i, n in enumerate(names)}
    c = {"FusedModel accepts" if chain(spec) else "FusedModel refuses"}

    def single(name, kind):
        i = prod.get(name)
        return i if i is not None and spec[i]["op"] == kind and len(cons.get(name, [])) == 1 else None

    def conv_bn(name):
        b = single(name, "bn")
        return single(srcs[b][0] if b is not None else name, "conv")

    for i, op in enumerate(spec):
        kind = op["op"]
        c.add("op %s" % kind + (" (new form)" if kind in ("maxpool", "avgpool") and new_pool(op) else ""))
        if kind in ("conv", "dense"):
            c.add("weights %s" % (op["kind"] + (str(op["nb"]) if op["kind"] == "quantized" else "")))
        if kind == "conv" and dilation(op) != (1, 1):
            c.add("dilated conv")
        if kind != "act":
            continue
        c.add("act %s" % op["fn"])
        # readers of the activation through the ops that keep codes
        wants, todo, through_flatten = set(), [(names[i], False)], False
        while todo:
            name, flat = todo.pop()
            for ci in cons.get(name, []):
                o = spec[ci]
                if o["op"] in ("conv", "dense"):
                    wants.add(_wclass(o))
                    bits = 1 if op["fn"] == "binary_tanh" else op.get("nb", 4)
                    mine = "bin" if bits == 1 else "i4" if bits <= 4 else "i8"
                    if flat and o["op"] == "dense" and ("bin", "i4", "i8", "f32").index(_wclass(o)) > ("bin", "i4", "i8").index(mine) \
                            and _wclass(o) != "f32":
                        through_flatten = True
                elif o["op"] == "flatten" or (o["op"] in ("maxpool", "globalmaxpool") and new_pool(o)):
                    todo.append((names[ci], flat or o["op"] == "flatten"))
        if len(wants - {"f32"}) > 1:
            c.add("one tensor, two stores wanted")
        if through_flatten:
            c.add("flatten before wider dense")
        # what is merged in front of it
        pre = srcs[i][0]
        sc = single(pre, "scale")
        ad = single(srcs[sc][0] if sc is not None else pre, "add")
        if ad is None:
            continue
        a_n, b_n = srcs[ad]
        for main, short in ((b_n, a_n), (a_n, b_n)):
            ci = conv_bn(main)
            if ci is None:
                continue
            si = prod.get(short)
            so = spec[si] if si is not None else {"op": "input"}
            if so["op"] == "act":
                bits = 1 if so["fn"] == "binary_tanh" else so.get("nb", 4)
                c.add("shortcut %s" % ("ternary" if so["fn"] == "ternary_tanh" else "float32 act" if so["fn"] == "leaky_relu"
                                        else "bin" if bits == 1 else "i4" if bits <= 4 else "i8"))
            elif so["op"] in ("bn", "conv"):
                c.add("shortcut float32 %s" % so["op"])
            else:
                c.add("shortcut other")
            p = _projection(spec, names, cons, prod, ci, short, i)
            if p is not None:
                c.add("projection %s" % p)
            break
    # classifier tails: avgpool -> flatten -> dense [-> softmax]
    for i, op in enumerate(spec):
        if op["op"] != "avgpool":
            continue
        fl = [k for k in cons.get(names[i], []) if spec[k]["op"] == "flatten"]
        de = [k for f in fl for k in cons.get(names[f], []) if spec[k]["op"] == "dense"]
        if not de:
            continue
        sm = [k for k in cons.get(names[de[0]], []) if spec[k]["op"] == "softmax"]
        end = sm[0] if sm else de[0]
        fused = (not new_pool(op) and len(cons.get(names[i], [])) == 1 and len(cons.get(names[fl[0]], [])) == 1 and
                 len(cons.get(names[de[0]], [])) == len(sm) and end == len(spec) - 1 and
                 spec[prod[srcs[i][0]]]["op"] == "act" and spec[prod[srcs[i][0]]]["fn"] in
                 ("binary_tanh", "quantized_tanh", "quantized_relu", "quantized_leakyrelu"))
        c.add("tail fused" if fused else "tail declined")
    return c


REQUIRED = ({"op %s" % k for k in ("conv", "dense", "bn", "act", "add", "scale", "flatten", "softmax", "zeropad", "maxpool",
                                   "avgpool", "maxpool (new form)", "avgpool (new form)", "globalmaxpool", "globalavgpool")} |
            {"act %s" % f for f in ("binary_tanh", "quantized_tanh", "quantized_relu", "quantized_leakyrelu", "ternary_tanh",
                                    "leaky_relu", "quantized_maxrelu", "quantized_leakymaxrelu")} |
            {"weights %s" % k for k in ("binary", "ternary", "float", "quantized2", "quantized3", "quantized4", "quantized8")} |
            {"shortcut %s" % k for k in ("i4", "bin", "i8", "ternary", "float32 bn", "float32 conv")} |
            {"one tensor, two stores wanted", "flatten before wider dense", "projection eligible", "projection near miss",
             "tail fused", "tail declined", "FusedModel accepts", "FusedModel refuses", "dilated conv"})
