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
Further down: the wide vocabulary (concat, the new-form spatial ops, dwconv, tconv: plan, HAND_WIDE, generate_wide) and the
grouped convolution (gconv: HAND_GROUPED, generate_grouped, REQUIRED_GROUPED).

Exactness by construction: images lie on k / 8, every weight is drawn on its own grid (so the layers' quantizers are
the identity) and a low-bit activation sits in front of every later contraction, with only max-pools, flattens, zero
padding and power-of-two-area averages in between.  Every product is then a multiple of one power of two and every sum
of magnitudes stays below 2^24 of them, so each contraction is exact in float32 in any order (guard checks it); what
is behind a contraction (bias, BN, add, scale, clip) is the same float32 op sequence everywhere."""
import numpy as np

from oracle import qnn_oracle as O

import conv_dilation_cases as D
import depthwise_cases as DW
import gconv_cases as GC
import maxrelu_cases as M
import pool_cases as P
import qrelu_cases as Q
import tconv_cases as TC

F32 = np.float32
N = 3
POOLS = ("maxpool", "avgpool", "globalmaxpool", "globalavgpool")


# ---- reading a spec -----------------------------------------------------------------------------------------------------
def names_of(spec):
    return [op.get("dst", "t%d" % i) for i, op in enumerate(spec)]


def sources(spec):
    """The tensors every op reads: add -> a, b; concat -> its srcs; a named `src`; else the previous op's output; else
    the images."""
    names = names_of(spec)
    return [[op["a"], op["b"]] if op["op"] == "add" else list(op["srcs"]) if op["op"] == "concat" else
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


def spatial_desc(op):
    """The crop / repeat / pad descriptor (spatial_cases.desc) of a new-form spatial op, or None: `crop`, `upsample`, and
    `zeropad` whose pad is ((top, bottom), (left, right)) rather than one integer."""
    ident = {"crop": ((0, 0), (0, 0)), "up": (1, 1), "pad": ((0, 0), (0, 0))}
    if op["op"] == "zeropad" and not isinstance(op["pad"], (int, np.integer)):
        return dict(ident, pad=op["pad"])
    if op["op"] == "crop":
        return dict(ident, crop=op["crop"])
    if op["op"] == "upsample":
        return dict(ident, up=tuple(op["size"]))
    return None


def dw_dilation(op):
    """A dwconv op and a gconv op carry their dilation as `dilation`."""
    return P.pair(op.get("dilation", (1, 1)))


def _stride(op):
    sh, sw = op.get("strides", (1, 1))
    assert sh == sw, "dwconv / tconv / gconv take one stride for both axes"
    return int(sh)


def _depthwise_transposed_or_grouped(op, src):
    """dwconv / tconv / gconv: the integer sum (depthwise_cases.dw_sum / tconv_cases.tconv_sum / gconv_cases.gconv_sum) on
    the exact integer codes of input and weights, scaled by their power of two, plus the bias in float32.  Operands that
    are no dyadic numbers (guard refuses such a case) are summed in float64 and rounded once.  weights(op) applies the
    quantizer to the whole kernel as the spec holds it; for a gconv that is Keras' grouped kernel (kh, kw, Cin / groups,
    Cout), so the ternary cutoff 0.7 mean|w| is taken over that whole kernel and never over a block-diagonal expansion:
    what the entry promises (include/qnn_abi_gconv.h)."""
    w = weights(op)
    try:
        (xc, a), (wc, b) = _codes(src, "input"), _codes(w, "weights")
        v = (_contract(xc, wc, op).astype(F32) * F32(2.0 ** -(a + b))).astype(F32)
    except ValueError:
        same = op.get("padding", "same") == "same"
        v = (DW.dw_sum(src, w, _stride(op), same, dw_dilation(op), np.float64) if op["op"] == "dwconv" else
             GC.gconv_sum(src, w, int(op["groups"]), _stride(op), same, dw_dilation(op), np.float64) if op["op"] == "gconv" else
             TC.tconv_sum(src, w, _stride(op), same, np.float64)).astype(F32)
    if op.get("bias") is not None:
        v = (v + np.asarray(op["bias"], dtype=F32)).astype(F32)
    return v


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
            elif kind == "concat":
                y = np.concatenate([env[s] for s in op["srcs"]], axis=-1)
            elif spatial_desc(op) is not None:
                import spatial_cases                         # (it imports this module)
                y = spatial_cases.spatial_array(src, spatial_desc(op))
            elif kind in ("dwconv", "tconv", "gconv"):
                y = _depthwise_transposed_or_grouped(op, src)
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
    if op["op"] == "dwconv":
        return DW.dw_sum(x, w, _stride(op), op.get("padding", "same") == "same", dw_dilation(op))
    if op["op"] == "tconv":
        return TC.tconv_sum(x, w, _stride(op), op.get("padding", "same") == "same")
    if op["op"] == "gconv":
        return GC.gconv_sum(x, w, int(op["groups"]), _stride(op), op.get("padding", "same") == "same", dw_dilation(op))
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
        if op["op"] in ("conv", "dense", "dwconv", "tconv", "gconv"):
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
            if op["op"] == "tconv":
                kh, kw, _, cin = wc.shape
                if TC.int32_refused(kh, kw, _stride(op), cin, a + 1, b):
                    return "op %d: the transposed convolution's int32 bound" % i
            if op["op"] == "gconv":
                kh, kw, cg, _ = wc.shape
                if GC.int32_refused(kh, kw, cg, a + 1, b):
                    return "op %d: the grouped convolution's int32 bound" % i
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

    # -- concat, the new-form spatial ops, dwconv and tconv
    def concat(self, srcs, dst=None):
        shapes = [self.shape[s] for s in srcs]
        assert len({s[:-1] for s in shapes}) == 1, shapes
        op = {"op": "concat", "srcs": list(srcs)}
        if dst is not None:
            op["dst"] = dst
        self.spec.append(op)
        name = names_of(self.spec)[-1]
        assert name not in self.shape, name
        self.shape[name] = shapes[0][:-1] + (sum(s[-1] for s in shapes),)
        self.cur = name
        return name

    def _spatial(self, op, src, dst):
        h, w, c = self.shape[self.cur if src is None else src]
        d = spatial_desc(op)                 # crop, then repeat, then pad (spatial_cases.out_hw; that module imports this one)
        ho = (h - sum(d["crop"][0])) * d["up"][0] + sum(d["pad"][0])
        wo = (w - sum(d["crop"][1])) * d["up"][1] + sum(d["pad"][1])
        assert ho > 0 and wo > 0
        return self._put(op, src, (ho, wo, c), dst)

    def zeropad2(self, pad, src=None, dst=None):
        return self._spatial({"op": "zeropad", "pad": pad}, src, dst)

    def crop(self, crop, src=None, dst=None):
        return self._spatial({"op": "crop", "crop": crop}, src, dst)

    def upsample(self, size, src=None, dst=None):
        return self._spatial({"op": "upsample", "size": size}, src, dst)

    def _bias(self, n, bias):
        """None, the float bias of conv(), or ("dyadic") multiples of 1 / 16: the sums stay dyadic without a clip."""
        if bias == "dyadic":
            return (self.rng.integers(-8, 9, n) / 16.0).astype(F32)
        return (self.rng.standard_normal(n) * 0.05).astype(F32) if bias else None

    def dwconv(self, M=1, kind="quantized", nb=4, k=3, s=1, pad="same", dil=1, bias=False, src=None, dst=None):
        """Keras' DepthwiseConv2D: kernel (kh, kw, C, M)."""
        h, w, c = self.shape[self.cur if src is None else src]
        (kh, kw), (dh, dw) = P.pair(k), P.pair(dil)
        op = {"op": "dwconv", "kind": kind, "kernel": _kernel(self.rng, kind, nb, (kh, kw, c, M)),
              "bias": self._bias(c * M, bias), "strides": (s, s), "padding": pad, "dilation": (dh, dw),
              "depth_multiplier": M, "H": 1.0}
        if kind == "quantized":
            op["nb"] = nb
        ho, wo = DW.out_pad(h, kh, s, pad == "same", dh)[0], DW.out_pad(w, kw, s, pad == "same", dw)[0]
        assert ho > 0 and wo > 0
        self.fan = kh * kw * _WVAR[kind]
        return self._put(op, src, (ho, wo, c * M), dst)

    def tconv(self, cout, kind="quantized", nb=4, k=2, s=2, pad="same", bias=False, src=None, dst=None):
        """Keras' Conv2DTranspose: kernel (kh, kw, Cout, Cin)."""
        h, w, cin = self.shape[self.cur if src is None else src]
        kh, kw = P.pair(k)
        op = {"op": "tconv", "kind": kind, "kernel": _kernel(self.rng, kind, nb, (kh, kw, cout, cin)),
              "bias": self._bias(cout, bias), "strides": (s, s), "padding": pad, "H": 1.0}
        if kind == "quantized":
            op["nb"] = nb
        ho, wo = TC.out_pad(h, kh, s, pad == "same")[0], TC.out_pad(w, kw, s, pad == "same")[0]
        self.fan = -(-kh // s) * -(-kw // s) * cin * _WVAR[kind]
        return self._put(op, src, (ho, wo, cout), dst)

    def gconv(self, cout, kind="quantized", nb=4, groups=1, k=3, s=1, dil=1, pad="same", bias=False, src=None, dst=None):
        """Keras' Conv2D(groups=g) as the importer emits it: kernel (kh, kw, Cin / groups, Cout)."""
        h, w, cin = self.shape[self.cur if src is None else src]
        (kh, kw), (dh, dw) = P.pair(k), P.pair(dil)
        assert cin % groups == 0 and cout % groups == 0, (cin, cout, groups)
        op = {"op": "gconv", "kind": kind, "kernel": _kernel(self.rng, kind, nb, (kh, kw, cin // groups, cout)),
              "bias": self._bias(cout, bias), "groups": groups, "strides": (s, s), "padding": pad, "dilation": (dh, dw),
              "H": 1.0}
        if kind == "quantized":
            op["nb"] = nb
        ho, wo = GC.out_pad(h, kh, s, pad == "same", dh)[0], GC.out_pad(w, kw, s, pad == "same", dw)[0]
        assert ho > 0 and wo > 0
        self.fan = kh * kw * (cin // groups) * _WVAR[kind]
        return self._put(op, src, (ho, wo, cout), dst)

    def dyadic_bn(self, src=None, dst=None):
        """Constants that are powers of two and multiples of 1 / 32 (eps 0, mean 0, variance 1, so inv = gamma and
        shift = beta exactly): what is behind it stays dyadic without a clip."""
        shape = self.shape[self.cur if src is None else src]
        c, rng = shape[-1], self.rng
        lo = -1 - int(np.log2(max(self.fan, 1.0))) // 2
        op = dict(op="bn", eps=0.0, gamma=((2.0 ** rng.integers(lo, lo + 2, c)) * rng.choice([-1.0, 1.0], c)).astype(F32),
                  beta=(rng.integers(-8, 9, c) / 32.0).astype(F32), mean=np.zeros(c, F32), var=np.ones(c, F32))
        return self._put(op, src, shape, dst)

    # a few groups the cases below repeat
    def group(self, cout, kind="quantized", nb=4, fn="quantized_tanh", abits=4, **kw):
        self.conv(cout, kind, nb, **kw)
        self.bn()
        return self.act(fn, abits)

    def clipped(self, cout, w="q4", a="q4", dst=None, bn=True, **kw):
        """conv -> [bn] -> clip by the names of WEIGHT_OF / ACT_OF; `dst` names the clip."""
        self.conv(cout, *WEIGHT_OF[w], **kw)
        if bn:
            self.bn()
        return self.act(*ACT_OF[a], dst=dst)

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


# ============================================================================================================================
# The wide vocabulary: concat, crop / upsample / pair-form zeropad, dwconv, tconv.
#
#   plan(spec)            GraphModel's planner restated on symbols: per tensor whether it travels as packed codes, as a
#                         clip not yet applied or as float32, the launches GraphModel.kernel_log records, and the
#                         decisions taken on the way (what categories() counts)
#   HAND_WIDE             one spec per planner decision, with the log the GPU file expects
#   generate_wide(seed)   random encoder-decoders, separable blocks, dense-net growth and inception branches
# ============================================================================================================================
_STORE_NAME = {0: "f32", 1: "bin", 2: "t2", 4: "i4", 8: "i8"}
_FN_OF = {"binary_tanh": "bin", "quantized_tanh": "qtanh", "quantized_relu": "qrelu", "quantized_leakyrelu": "qleaky"}
_DWFN = {"bin": DW.FN_BINARY_TANH, "qtanh": DW.FN_QUANTIZED_TANH, "qrelu": DW.FN_QUANTIZED_RELU,
         "qleaky": DW.FN_QUANTIZED_LEAKYRELU}


def _wstore(op):
    """Narrowest packed store of a contraction's weights (1 / 4 / 8), None for float or 16-bit weights."""
    if op["kind"] == "binary":
        return 1
    if op["kind"] == "ternary":
        return 4
    if op["kind"] == "quantized" and op["nb"] <= 8:
        return 4 if op["nb"] <= 4 else 8
    return None


def _bits_store(bits):
    return 1 if bits == 1 else 4 if bits <= 4 else 8


def _join(bits, wstore):
    """The store both operands of a contraction are brought to (engine._join_store)."""
    if wstore is None:
        return None
    a = _bits_store(bits)
    if a == 1 and wstore == 1:
        return 1
    return max(0 if a == 1 else a, 0 if wstore == 1 else wstore, 4)


def _grid_store(op):
    """The store a contraction reads ternary codes {-1, 0, 1} at (engine.GraphModel._grid_store)."""
    ws = _wstore(op) if op["op"] in ("conv", "dense", "dwconv", "tconv", "gconv") else None
    if ws is None:
        return None
    return 2 if op["kind"] == "ternary" else max(4, ws if ws != 1 else 4)


def _clip_of(op):
    """(fn, bits) of an activation op that is a low-bit clip, else None (engine._act_code)."""
    if op["fn"] == "binary_tanh":
        return "bin", 1
    if op["fn"] in _FN_OF and op["nb"] <= 8:
        return _FN_OF[op["fn"]], int(op["nb"])
    return None


def _F(ndim):
    return {"k": "F", "ndim": ndim}


def _V(fn, nb, ndim, origin=None):
    return {"k": "V", "fn": fn, "nb": nb, "ndim": ndim, "origin": origin}


def _P(store, bits, ndim, grid=False, origin=None):
    return {"k": "P", "store": store, "bits": bits, "grid": grid, "ndim": ndim, "origin": origin}


def _shapes(spec, hw_c):
    """name -> shape without the batch axis, from the reference on one zero image."""
    env = reference(spec, np.zeros((1,) + tuple(hw_c), F32), return_all=True)
    return {k: v.shape[1:] for k, v in env.items()}


def plan(spec, image=(8, 8, 3)):
    """(state per tensor, kernel_log, decisions) of GraphModel(spec) without scaled codes.  kernel_log: what the engine
    appends to GraphModel.kernel_log; decisions: a set of strings."""
    names, srcs, cons = names_of(spec), sources(spec), consumers(spec)
    prod = {n: i for i, n in enumerate(names)}
    shape = _shapes(spec, image)
    env, log, dec, skip, upsampled = {"input": _F(4)}, [], set(), set(), set()

    def origin_tags(st, through):
        """Categories of codes going through a spatial op or a concat."""
        dec.add("codes through %s: %s" % (through, _STORE_NAME[st["store"]]))
        o = st.get("origin")
        if o is not None:
            fn, nb = o
            for tag, hit in (("relu", fn == "qrelu"), ("leaky", fn == "qleaky"), ("2-bit", nb == 2 and fn != "bin"),
                             ("3-bit", nb == 3)):
                if hit:
                    dec.add("%s codes through a spatial op or concat" % tag)

    def grid_plan(name):
        stores, todo, looked = set(), [name], False
        while todo:
            n = todo.pop()
            if n == names[-1]:
                return None
            for c in cons.get(n, []):
                o = spec[c]
                if o["op"] == "concat" or spatial_desc(o) is not None:
                    todo.append(names[c])
                    looked |= o["op"] == "concat"
                else:
                    stores.add(_grid_store(o))
        if len(stores) > 1 and None not in stores and looked:
            dec.add("ternary: no common store behind a concat")
        return stores.pop() if len(stores) == 1 else None

    def pack_clip(v, name=None):
        if v["k"] != "V" or v["ndim"] != 4:
            return None
        if v["fn"] == "grid":
            store = grid_plan(name) if name is not None else None
            return None if store is None else _P(store, 1, 4, True, ("grid", 1))
        bits = 1 if v["fn"] == "bin" else v["nb"]
        return _P(_bits_store(bits), bits, 4, False, (v["fn"], v["nb"]))

    def read_packed(i, op, src, ndim):
        """A contraction on packed codes: True if it reads them as they are, else the re-clip branch."""
        ws = _wstore(op)
        want = _grid_store(op) if src["grid"] else _join(src["bits"], ws) if ws is not None else None
        if ws is not None and want == src["store"] and src["ndim"] == ndim:
            return True
        if ws is not None:
            dec.add("packed producer, other store wanted")
        return False

    def depth(i, op, src):
        kind, last = op["op"], i
        if cons.get(names[last], []) == [last + 1] and spec[last + 1]["op"] == "bn":
            last += 1
        elif any(spec[c]["op"] == "bn" for c in cons.get(names[i], [])) and len(cons.get(names[i], [])) > 1:
            dec.add("a second reader beside the BN behind %s" % kind)
        if last > i and len(cons.get(names[last], [])) > 1:
            dec.add("BN behind %s read twice" % kind)
        out = None
        if last + 1 < len(spec) and cons.get(names[last], []) == [last + 1] and spec[last + 1]["op"] == "act" and \
                _clip_of(spec[last + 1]) is not None:
            out = _clip_of(spec[last + 1])
            last += 1
            dec.add("%s clip in the epilogue" % kind)
            for c in cons.get(names[last], []):
                dec.add("packed %s output read by %s" % (kind, spec[c]["op"] + (" (new form)" if new_pool(spec[c]) and
                                                                                 spec[c]["op"] in ("maxpool", "avgpool") else "")))
            if names[last] == names[-1]:
                dec.add("packed %s output is the last tensor" % kind)
            if len(cons.get(names[last], [])) > 1:
                dec.add("clip behind %s read twice" % kind)
        ws = _wstore(op)
        xs, xbits = 0, 0
        if src["k"] == "P":
            if read_packed(i, op, src, 4):
                xs, xbits = src["store"], src["bits"]
            else:
                src = _V("grid" if src["grid"] else "bin" if src["store"] == 1 else "qtanh", src["bits"], src["ndim"])
        if xs == 0 and src["k"] == "V" and ws is not None and src["ndim"] == 4:
            if src["fn"] == "grid":
                xs, xbits = _grid_store(op), 1
            else:
                xbits = 1 if src["fn"] == "bin" else src["nb"]
                xs = _join(xbits, ws)
            log.append("pack")
        # the kernel's name
        kh, kw = op["kernel"].shape[:2]
        wshift = op["nb"] - 1 if op["kind"] == "quantized" else 0
        ostore = 0 if out is None else _bits_store(out[1])
        suffix = ""
        if kind == "dwconv" and xs in (4, 8):
            pk16 = DW.takes_pk16(dict(store=xs, out_store=ostore, M=op["kernel"].shape[3], window=(kh, kw), stride=_stride(op),
                                      dil=dw_dilation(op), x_bits=xbits, wkind=DW.W_QUANT if op["kind"] == "quantized" else 1,
                                      wbits=op.get("nb", 1)))
            suffix = "" if pk16 else "_plain"
            if pk16:
                dec.add("depthwise 16-bit-lane form")
        elif kind == "tconv" and xs in (4, 8):
            mfma = TC.takes_mfma(dict(window=(kh, kw), stride=_stride(op), store=xs, out_store=ostore, Cin=op["kernel"].shape[3],
                                      Cout=op["kernel"].shape[2], misalign=False))
            suffix = "_mfma" if mfma else "_plain"
            if mfma:
                dec.add("tconv matrix-pipe form")
        elif kind == "gconv" and xs in (4, 8):
            cg, cout = op["kernel"].shape[2:]
            route = dict(window=(kh, kw), store=xs, out_store=ostore, Cin=cg * int(op["groups"]), Cout=cout,
                         groups=int(op["groups"]), misalign=False)
            mfma = GC.takes_mfma(route)
            suffix = "_mfma" if mfma else "_plain"
            if mfma:
                dec.add("gconv matrix-pipe form")
            elif GC.takes_mfma(dict(route, out_store=xs)):   # the shape is the matrix pipe's, the epilogue leaves another store
                dec.add("gconv plain form: other out store")
        log.append("%s_%s%s" % ({"dwconv": "depthwise", "tconv": "tconv", "gconv": "gconv"}[kind], _STORE_NAME[xs], suffix))
        y = _F(4) if out is None else _P(ostore, out[1], 4, False, out)
        return y, last

    for i, op in enumerate(spec):
        if i in skip:
            continue
        kind, name = op["op"], names[i]
        src = env[srcs[i][0]]
        pi = prod.get(srcs[i][0])
        if pi is not None and spec[pi]["op"] == "act" and spec[pi]["fn"] in M.FNS:
            for tag, hit in (("dwconv", kind == "dwconv"), ("tconv", kind == "tconv"), ("gconv", kind == "gconv"),
                             ("spatial", spatial_desc(op) is not None)):
                if hit:
                    dec.add("max activation in front of %s" % tag)
        if kind == "concat" and any(prod.get(s) is not None and spec[prod[s]]["op"] == "act" and spec[prod[s]]["fn"] in M.FNS
                                    for s in srcs[i]):
            dec.add("max activation in front of concat")
        if kind == "avgpool" and not new_pool(op) and src["k"] == "V" and src["fn"] != "grid" and _tail_at(spec, names, cons, i):
            t = _tail_at(spec, names, cons, i)
            skip.update(t)
            name, y = names[max(t)], _F(2)
        elif kind in ("conv", "dense"):
            if cons.get(name, []) == [i + 1] and spec[i + 1]["op"] == "bn":
                skip.add(i + 1)
                name = names[i + 1]
            if src["k"] == "P":
                read_packed(i, op, src, 4 if kind == "conv" else 2)
            y = _F(4 if kind == "conv" else 2)
        elif kind in ("dwconv", "tconv", "gconv"):
            y, last = depth(i, op, src)
            skip.update(range(i + 1, last + 1))
            name = names[last]
            if kind in ("tconv", "gconv") and y["k"] == "P":
                upsampled.add(name)
        elif kind == "concat":
            ins = [env[s] for s in srcs[i]]
            pack_clips = any(s in upsampled or (s in prod and spatial_desc(spec[prod[s]]) is not None) for s in srcs[i])
            if pack_clips and any(t["k"] == "P" for t in ins):
                like = next(t for t in ins if t["k"] == "P")
                packs = [t if t["k"] == "P" else None if t["k"] != "V" else
                         (_P(like["store"], 1, 4, True, ("grid", 1)) if like["grid"] and t["ndim"] == 4 else None)
                         if t["fn"] == "grid" else pack_clip(t) for t in ins]
                if all(p is not None for p in packs) and len({(p["store"], p["bits"], p["grid"]) for p in packs}) == 1:
                    if any(t["k"] == "V" for t in ins):
                        dec.add("pack_clips join")
                    ins = packs
            if all(t["k"] == "P" for t in ins) and len({(t["store"], t["bits"], t["grid"]) for t in ins}) == 1:
                dec.add("concat join: codes")
                for t in ins:
                    origin_tags(t, "concat")
                log.append("concat_" + _STORE_NAME[ins[0]["store"]])
                y = _P(ins[0]["store"], ins[0]["bits"], ins[0]["ndim"], ins[0]["grid"], ins[0]["origin"])
            elif all(t["k"] == "V" for t in ins) and len({(t["fn"], t["nb"]) for t in ins}) == 1:
                dec.add("concat join: clips")
                log.append("concat_f32")
                y = _V(ins[0]["fn"], ins[0]["nb"], ins[0]["ndim"])
            else:
                dec.add("concat join: float32")
                if any(t["k"] == "P" for t in ins) and any(t["k"] == "V" for t in ins):
                    dec.add("concat: codes meet a clip, joined in float32")
                log.append("concat_f32")
                y = _F(ins[0]["ndim"])
        elif spatial_desc(op) is not None:
            padded = kind == "zeropad"
            if src["k"] == "V" and not (padded and src["fn"] == "bin"):
                src = pack_clip(src, name) or src
            if src["k"] == "P" and src["ndim"] == 4 and not (padded and src["store"] == 1):
                origin_tags(src, kind)
                log.append("spatial_" + _STORE_NAME[src["store"]])
                y = _P(src["store"], src["bits"], 4, src["grid"], src["origin"])
            else:
                if src["k"] == "P":
                    log.append("unpack")
                log.append("spatial_f32")
                y = _F(4)
        elif kind == "act" and _clip_of(op) is not None:
            y = _V(*_clip_of(op), src["ndim"])
        elif kind == "act" and op["fn"] == "ternary_tanh":
            y = _V("grid", 1, src["ndim"])
        elif kind in POOLS and new_pool(op):
            mode = "max" if "max" in kind else "avg"
            if src["k"] == "V" and src["fn"] != "grid" and src["ndim"] == 4:
                src = pack_clip(src)
            if src["k"] == "P" and src["ndim"] == 4:
                log.append("pool_%s_%s" % (mode, _STORE_NAME[src["store"]]))
                if src.get("origin") is not None and prod.get(srcs[i][0]) is not None and \
                        spec[prod[srcs[i][0]]]["op"] == "act" and _epilogue_of(spec, names, cons, prod[srcs[i][0]]):
                    dec.add("pool on the codes of a dwconv / tconv")
                y = _P(src["store"], src["bits"], 2 if kind.startswith("global") else 4, False, src["origin"]) if mode == "max" \
                    else _F(2 if kind.startswith("global") else 4)
            else:
                log.append("pool_%s_f32" % mode)
                y = _F(2 if kind.startswith("global") else 4)
        elif kind == "flatten":
            y = _F(2)
        else:                                                # bn, add, scale, softmax, the other activations, old-form pools and pads
            y = _F(src["ndim"])
        env[name] = y
    return env, log, dec


def _tail_at(spec, names, cons, ap):
    """The ops (flatten, dense[, softmax]) the classifier tail at old-form avgpool `ap` takes with it, or ()."""
    def only(i, kind):
        c = cons.get(names[i], []) if i is not None else []
        return c[0] if len(c) == 1 and spec[c[0]]["op"] == kind else None
    fl = only(ap, "flatten")
    de = only(fl, "dense")
    if de is None:
        return ()
    sm = only(de, "softmax")
    if sm is None:
        return (fl, de) if de == len(spec) - 1 and not cons.get(names[de]) else ()
    return (fl, de, sm) if len(cons.get(names[de], [])) == 1 and not cons.get(names[sm]) else ()


def _epilogue_of(spec, names, cons, ai):
    """True if activation op `ai` goes into the epilogue of a dwconv / tconv / gconv (alone behind it or behind its BN)."""
    srcs = sources(spec)
    prod = {n: i for i, n in enumerate(names)}
    p = prod.get(srcs[ai][0])
    if p is None or p != ai - 1 or cons.get(names[p], []) != [ai]:
        return False
    if spec[p]["op"] == "bn":
        q = prod.get(srcs[p][0])
        return q == p - 1 and spec[q]["op"] in ("dwconv", "tconv", "gconv") and cons.get(names[q], []) == [p]
    return spec[p]["op"] in ("dwconv", "tconv", "gconv")


# ---- hand-written specs, one per planner decision ---------------------------------------------------------------------------
HAND_WIDE = []


def _wide(name, net, log=None, layer_model=None):
    """log: the launches GraphModel.kernel_log must hold, in order, written out by hand (None: plan()'s prediction alone
    is asserted, as for every spec).  layer_model: "float conv" where LayerModel answers with its low-bit-only error."""
    assert name not in [c["name"] for c in HAND_WIDE], name
    HAND_WIDE.append(dict(name=name, spec=net.spec, x=net.images(), image=net.shape["input"], log=log, layer_model=layer_model))


def _head(net, w="q4", flat=True):
    if not flat:
        net.pool("globalmaxpool")
        return net.dense(10, *WEIGHT_OF[w], bias=True)
    return net.classifier(*WEIGHT_OF[w])


# GraphModel._spatial / _concat / _pack_clip: codes of every clip function and width through crop, upsample, pair zeropad
# and a concat with the skip (pack_clips packs the skip to meet them); bin: the pad runs in float32
_W_FOR = {"bin": "bin", "q2": "q2", "q3": "q4", "q4": "q4", "q8": "q8", "relu4": "q4", "relu8": "q8", "leaky4": "q4",
          "leaky2": "q2", "tern": "tern"}
for _a in ("bin", "q2", "q3", "q8", "relu4", "relu8", "leaky4", "leaky2", "tern"):
    _w = _W_FOR[_a]
    net = Net(_seed("through_" + _a), hw=(9, 7))
    a0 = net.clipped(8, _w, _a, dst="a0")
    net.crop(((1, 0), (0, 1)), src=a0, dst="cr")                      # 8 x 6
    net.pool("maxpool", (2, 2), (2, 2), "valid", dst="p")             # 4 x 3: on the codes the crop left
    a1 = net.clipped(12, _w, _a, dst="a1")
    net.upsample((2, 2), dst="up")                                    # 8 x 6
    net.concat(["up", "cr"], dst="cat")
    net.zeropad2(((0, 1), (1, 0)), dst="zp")                          # 9 x 7
    net.clipped(8, _w, _a, pad="valid")
    _head(net, _w)
    _wide("codes_through_%s" % _a, net)

# _dwconv / _tconv: the packed output of a fused clip read by everything but a matching conv
for _k in ("dwconv", "tconv"):
    def _producer(net, a="q4", w="q4", bn=True, dst="y"):
        if _k == "dwconv":
            net.dwconv(1, *WEIGHT_OF[w], bias=True)
        else:
            net.tconv(8, *WEIGHT_OF[w], k=3, s=1, bias=True)
        if bn:
            net.bn()
        return net.act(*ACT_OF[a], dst=dst)

    def _stem(name, hw=(8, 8), c=8, a="q4"):
        net = Net(_seed(name), hw=hw)
        net.clipped(c, "q4", a, dst="a0")
        return net

    # a new-form max-pool and a global max-pool: pooled on the codes
    net = _stem(_k + "_pool")
    _producer(net)
    net.pool("maxpool", (3, 3), (2, 2), "same")
    net.clipped(8)
    _head(net)
    _wide(_k + "_then_new_maxpool", net, log=["pack", "depthwise_i4" if _k == "dwconv" else "tconv_i4_plain", "pool_max_i4"])
    net = _stem(_k + "_gpool")
    _producer(net, a="q8")
    _head(net, "q8", flat=False)
    _wide(_k + "_then_global_maxpool", net)
    net = _stem(_k + "_avg")
    _producer(net)
    net.pool("avgpool", (2, 2), (2, 2), "valid")
    _head(net)
    _wide(_k + "_then_new_avgpool", net)
    # a spatial op, then a conv
    net = _stem(_k + "_spatial", hw=(9, 7))
    _producer(net, a="relu4")
    net.crop(((0, 1), (1, 0)))
    net.upsample((1, 2))
    net.clipped(8)
    _head(net)
    _wide(_k + "_then_spatial", net)
    # flatten -> dense, and the network's last tensor
    net = _stem(_k + "_flat", hw=(4, 4))
    _producer(net)
    _head(net)
    _wide(_k + "_then_flatten_dense", net)
    net = _stem(_k + "_last")
    _producer(net, a="leaky4")
    _wide(_k + "_clip_is_last", net)
    # add, bn
    net = _stem(_k + "_add")
    y = _producer(net)
    net.add("a0", y)
    net.scale(0.5)
    net.act()
    _head(net)
    _wide(_k + "_then_add", net)
    net = _stem(_k + "_bn")
    _producer(net, bn=False)
    net.bn()
    net.act()
    _head(net)
    _wide(_k + "_then_bn", net)
    # two consumers that want different stores; a contraction whose join store differs (the re-clip branch)
    net = _stem(_k + "_two")
    y = _producer(net)
    net.conv(8, "quantized", 4, src=y)
    b1 = net.bn()
    net.conv(8, "quantized", 8, src=y)
    b2 = net.bn()
    net.add(b1, b2)
    net.act()
    _head(net)
    _wide(_k + "_two_consumers_two_stores", net)
    net = _stem(_k + "_reclip")
    _producer(net, a="bin")
    net.dwconv(2, "quantized", 8, k=(2, 3))                           # 1-bit codes, 8-bit weights: another store
    net.bn()
    net.act("quantized_tanh", 8)
    _head(net, "q8")
    _wide(_k + "_other_store_wanted", net)
    # the BN behind it read twice stays a tensor; the clip behind it read twice is still fused
    net = _stem(_k + "_bn2")
    _producer(net, bn=False, dst="y0")
    net2 = net                                                        # (the producer without a BN, then one read twice)
    net = _stem(_k + "_bn_twice")
    if _k == "dwconv":
        net.dwconv(1, bias=True)
    else:
        net.tconv(8, k=3, s=1, bias=True)
    b = net.bn(dst="b")
    a1 = net.act(src=b, dst="a1")
    net.clipped(8, src=a1, dst="a2")
    net.act("quantized_tanh", 8, src=b, dst="a3")
    net.concat(["a2", "a3"])
    net.clipped(8)
    _head(net)
    _wide(_k + "_bn_read_twice", net)
    net = _stem(_k + "_clip_twice")
    y = _producer(net)
    net.pool("maxpool", (2, 2), (2, 2), "valid", src=y, dst="p")
    net.clipped(8, s=2, src=y, dst="c")
    net.concat(["p", "c"])
    net.clipped(8)
    _head(net)
    _wide(_k + "_clip_read_twice", net)
    # a batch-maximum activation in front: always read as float32
    net = Net(_seed(_k + "_max"), hw=(8, 8))
    net.conv(8, bias=True)
    net.act("quantized_maxrelu", 4)
    _producer(net)
    net.clipped(8)
    _head(net)
    _wide(_k + "_behind_max_activation", net)
    # ternary weights reading grid codes; float kind (LayerModel takes it, while it refuses a float conv)
    net = Net(_seed(_k + "_tern"), hw=(8, 8))
    net.clipped(8, "tern", "tern")
    _producer(net, a="tern", w="tern")
    net.clipped(8, "tern", "tern")
    _head(net, "tern")
    _wide(_k + "_ternary_on_grid_codes", net)
    net = Net(_seed(_k + "_float"), hw=(8, 8))
    if _k == "dwconv":
        net.dwconv(2, "float", 0, s=2, bias="dyadic")
    else:
        net.tconv(5, "float", 0, k=3, s=2, pad="valid", bias="dyadic")
    net.act()
    net.clipped(8)
    _head(net)
    _wide(_k + "_float_kind", net)

# _concat: a dwconv's packed codes meet an unmaterialised clip: pack_clips is false, the join falls to float32 ...
net = Net(_seed("dw_meets_clip"), hw=(8, 8))
a0 = net.clipped(8, dst="a0")
net.dwconv(1, bias=True)
net.bn()
net.act(dst="d")
net.concat(["d", "a0"])
net.clipped(8)
_head(net)
_wide("dwconv_codes_meet_a_clip", net, log=["pack", "depthwise_i4", "concat_f32"])
# ... and the same network with a tconv stays on codes
net = Net(_seed("tc_meets_clip"), hw=(8, 8))
a0 = net.clipped(8, dst="a0")
net.tconv(8, k=3, s=1, bias=True)
net.bn()
net.act(dst="d")
net.concat(["d", "a0"])
net.clipped(8)
_head(net)
_wide("tconv_codes_meet_a_clip", net, log=["pack", "tconv_i4_plain", "concat_i4"])

# tconv across a skip on the matrix pipe: a 64-channel 4 x 4 map, 2 x 2 / 2 and 4 x 4 / 2, int4 and int8
for _a, _k2 in (("q4", 2), ("q8", 4), ("q4", 3)):
    net = Net(_seed("unet_%s_%d" % (_a, _k2)), hw=(8, 8))
    a0 = net.clipped(16, _a, _a, dst="skip")
    net.pool("maxpool", 2)
    net.clipped(64, _a, _a)
    net.tconv(16, *WEIGHT_OF[_a], k=_k2, s=2, bias=True)
    net.bn()
    net.act(*ACT_OF[_a], dst="up")
    net.concat(["up", "skip"])
    net.clipped(16, _a, _a)
    _head(net, _a, flat=False)
    _s = {"q4": "i4", "q8": "i8"}[_a]
    _wide("tconv_skip_%s_k%d" % (_a, _k2), net, log=["pack", "tconv_%s_mfma" % _s, "concat_" + _s, "pool_max_" + _s])

# a depthwise block on the 16-bit lanes and on the plain form (dilated, strided, depth multiplier 2)
for _n, _kw in (("pk16", dict()), ("dilated", dict(dil=2)), ("strided_m2", dict(M=2, s=2, k=(2, 3))), ("k5", dict(k=5))):
    net = Net(_seed("sep_" + _n), hw=(9, 7))
    net.clipped(16, dst="a0")
    net.dwconv(bias=True, **_kw)
    net.bn()
    net.act()
    net.clipped(12, k=1)
    _head(net)
    _wide("separable_" + _n, net, log=["pack", "depthwise_i4" if _n == "pk16" else "depthwise_i4_plain"])

# _grid_plan: ternary activations behind a concat whose contractions disagree on the store (T2, I4 and I8) ...
net = Net(_seed("tern_no_store"), hw=(8, 8))
a0 = net.clipped(8, "tern", "tern", dst="a0")
a1 = net.clipped(8, "tern", "tern", dst="a1")
net.upsample((1, 1), src=a0, dst="u")
net.concat(["u", "a1"], dst="cat")
net.conv(8, "ternary", 1, src="cat")
b1 = net.bn()
net.conv(8, "quantized", 4, src="cat")
b2 = net.bn()
net.conv(8, "quantized", 8, src="cat")
b3 = net.bn()
net.add(b1, b2)
net.add(net.cur, b3)
net.act("ternary_tanh")
_head(net, "tern")
_wide("ternary_no_common_store", net, log=["spatial_f32", "concat_f32"])
# ... and where they agree (all ternary): planes through the up-sampling and the join
net = Net(_seed("tern_concat"), hw=(8, 8))
a0 = net.clipped(8, "tern", "tern", dst="a0")
net.pool("maxpool", 2)
net.clipped(12, "tern", "tern")
net.upsample((2, 2), dst="u")
net.concat(["u", "a0"], dst="cat")
net.clipped(8, "tern", "tern")
_head(net, "tern")
_wide("ternary_concat_on_planes", net, log=["spatial_t2", "concat_t2"])

# _concat's joins
net = Net(_seed("cat_fns"), hw=(8, 8))                       # one width, different functions: float32
a0 = net.clipped(8, dst="a0")
net.clipped(8, "q4", "q4", src=a0, dst="x")
net.clipped(8, "q4", "relu4", src=a0, dst="y")
net.concat(["x", "y"])
net.clipped(8)
_head(net)
_wide("concat_one_width_two_functions", net, log=["concat_f32"])
net = Net(_seed("cat_widths"), hw=(8, 8))                    # two widths in one store, as pooled codes: float32
a0 = net.clipped(8, dst="a0")
net.clipped(8, "q4", "q2", src=a0)
net.pool("maxpool", (2, 2), (2, 2), "valid", dst="x")
net.clipped(8, "q4", "q4", src=a0)
net.pool("maxpool", (2, 2), (2, 2), "valid", dst="y")
net.concat(["x", "y"])
net.clipped(8)
_head(net)
_wide("concat_two_widths_one_store", net, log=["pool_max_i4", "pool_max_i4", "concat_f32"])
net = Net(_seed("cat_twice"), hw=(8, 8))                     # one tensor twice, three inputs, a concat of a concat, last op
a0 = net.clipped(5, dst="a0")
a1 = net.clipped(3, src=a0, dst="a1")
net.concat(["a0", "a0"], dst="c1")
net.concat(["c1", "a1", "a0"], dst="c2")
net.clipped(8, src="c2", dst="a2")
net.concat(["a2", "c2", "a2", "a0"])
_wide("concat_twice_nested_and_last", net, log=["concat_f32"] * 3)
net = Net(_seed("cat_binpad"), hw=(8, 8))                    # a float32 pair zeropad behind a 1-bit clip beside packed codes
a0 = net.clipped(8, "bin", "bin", dst="a0")
net.crop(((1, 1), (1, 1)), src=a0, dst="c")
net.zeropad2(((1, 1), (1, 1)), dst="z")
net.pool("maxpool", (3, 3), (1, 1), "same", src=a0, dst="p")
net.concat(["z", "p"])
net.clipped(8, "bin", "bin")
_head(net, "bin")
_wide("binary_pad_beside_packed_branch", net, log=["spatial_bin", "unpack", "spatial_f32", "pool_max_bin", "concat_f32"])

# a batch-maximum activation in front of a spatial op and of a concat
net = Net(_seed("max_spatial"), hw=(8, 8))
net.conv(8, bias=True)
m = net.act("quantized_leakymaxrelu", 4, dst="m")
net.upsample((2, 1), dst="u")
net.crop(((4, 4), (0, 0)), dst="c")
net.concat(["c", "m"])
net.clipped(8)
_head(net)
_wide("max_activation_spatial_and_concat", net, log=["spatial_f32", "spatial_f32", "concat_f32"])

# LayerModel's domain protocol: the grid kept through crop / upsample, dropped at a zeropad; a float conv still refused
net = Net(_seed("lm_chain"), hw=(9, 7))
net.clipped(8, "q4", "q4")
net.crop(((1, 0), (0, 1)))
net.upsample((2, 2))
net.clipped(8, "q4", "q8")
net.zeropad2(((1, 1), (2, 0)))
net.clipped(8, "q8", "bin", pad="valid")
net.upsample((1, 2))
net.dwconv(1, "binary", 1, bias=True)
net.bn()
net.act("binary_tanh", 1)
_head(net, "bin")
_wide("layermodel_domains_through_spatial_ops", net)
net = Net(_seed("lm_float"), hw=(8, 8))
net.clipped(8)
net.upsample((2, 2))
net.conv(8, "float", 0, s=2)
net.bn()
net.act()
_head(net)
_wide("float_conv_behind_an_upsample", net, layer_model="float conv")

CAPTURED = ("tconv_skip_q4_k2", "separable_pk16", "ternary_concat_on_planes")

# ternary planes through a crop and a pair zeropad, each read by a ternary conv alone
net = Net(_seed("tern_crop_pad"), hw=(9, 7))
net.clipped(8, "tern", "tern")
net.crop(((1, 0), (0, 1)))
net.clipped(8, "tern", "tern")
net.zeropad2(((1, 1), (0, 2)))
net.clipped(8, "tern", "tern", pad="valid")
_head(net, "tern")
_wide("ternary_planes_through_crop_and_pad", net, log=["spatial_t2", "spatial_t2"])


# ---- the second generator ---------------------------------------------------------------------------------------------------
SEEDS_WIDE = range(64)
CHANNELS_WIDE = (3, 5, 8, 12, 16, 24, 32, 33, 64)
MAX_CONTRACTIONS_WIDE = 7


def generate_wide(seed):
    """(spec, images, image shape) of a random network over the wide vocabulary: a stem, 2 to 4 blocks out of {plain
    group, pool, identity residual, encoder-decoder with a concat skip, separable block, dense-net growth, inception
    branches}, some of them inside a residual add, and a head; weights and activations are drawn per op.  Seeds 0 mod 8
    hold the matrix-pipe transposed convolution, seeds 1 mod 8 the 16-bit-lane depthwise form."""
    rng = np.random.default_rng(70000 + seed)
    force = {0: "mfma", 1: "pk16"}.get(seed % 8)
    net = Net(60000 + seed, hw=(8, 8) if force == "mfma" or rng.random() < 0.5 else (9, 7))
    pick = lambda seq: seq[int(rng.integers(len(seq)))]      # noqa: E731
    use_max = force is None and rng.random() < 0.2
    left = [MAX_CONTRACTIONS_WIDE - 1]                       # (the head's dense is one)
    wkeys = ("bin", "tern", "q2", "q3", "q4", "q4", "q8")
    akeys = ("bin", "q2", "q3", "q4", "q4", "q8", "relu4", "relu8", "leaky4", "leaky2", "tern")
    small = tuple(c for c in CHANNELS_WIDE if c <= 33)

    def act(a=None):
        if a is None and use_max and rng.random() < 0.4:
            return net.act(pick(("quantized_maxrelu", "quantized_leakymaxrelu")), pick((3, 4)))
        return net.act(*ACT_OF[a or pick(akeys)])

    def clipped(cout, w=None, a=None, **kw):
        left[0] -= 1
        net.conv(cout, *WEIGHT_OF[w or pick(wkeys)], bias=bool(rng.random() < 0.5), **kw)
        if rng.random() < 0.8:
            net.bn()
        return act(a)

    def finish(a=None):
        """[bn] [clip] behind a dwconv / tconv: each present or absent; without a clip the constants are dyadic."""
        has_bn, has_clip = rng.random() < 0.7, a is not None or rng.random() < 0.8
        if has_bn:
            net.bn() if has_clip else net.dyadic_bn()
        return act(a) if has_clip else net.cur, has_clip

    def depthwise(src, M=None, k=None, s=None, dil=None, w=None, a=None):
        left[0] -= 1
        s = pick((1, 1, 2)) if s is None else s
        dil = (pick((1, 1, 2)) if s == 1 else 1) if dil is None else dil
        clip = a is not None or rng.random() < 0.8
        net.dwconv(pick((1, 1, 2)) if M is None else M, *WEIGHT_OF[w or pick(wkeys)], k=pick((3, 3, (2, 3), 5)) if k is None else k,
                   s=s, dil=dil, bias=(bool(rng.random() < 0.5) if clip else "dyadic"), src=src)
        if rng.random() < 0.7:
            net.bn() if clip else net.dyadic_bn()
        return act(a) if clip else net.cur

    def separable(cur, **kw):
        depthwise(cur, **kw)
        return clipped(pick(small), k=1)

    def encdec(cur, mfma=False):
        h, w_, c = net.shape[cur]
        up_kind = "tconv" if mfma else pick(("upsample", "tconv", "tconv"))
        k, s = (pick((2, 3, 4)), 2) if mfma else pick(((2, 2), (3, 2), (4, 2), (3, 1), (2, 3)))
        if up_kind == "upsample":
            s = 2
        a = pick(("q4", "q8")) if mfma else None
        if s == 1:
            mid = clipped(pick(small), src=cur)
        elif s == 3:
            net.pool("maxpool", (3, 3), (3, 3), "same", src=cur)
            mid = clipped(pick(small))
        elif mfma or rng.random() < 0.5:
            net.pool("maxpool", (2, 2), (2, 2), "same", src=cur)
            mid = clipped(64, a, a) if mfma else clipped(pick(small))
        else:
            mid = clipped(pick(small), s=2, src=cur)
        if up_kind == "upsample":
            up = net.upsample((2, 2))
        else:
            left[0] -= 1
            clip = mfma or rng.random() < 0.85
            net.tconv(pick((16, 32)) if mfma else pick(small), *WEIGHT_OF[a or pick(wkeys)], k=k, s=s,
                      bias=(bool(rng.random() < 0.5) if clip else "dyadic"))
            if rng.random() < 0.7:
                net.bn() if clip else net.dyadic_bn()
            up = act(a) if clip else net.cur
        dh, dw = net.shape[up][0] - h, net.shape[up][1] - w_
        assert dh >= 0 and dw >= 0, (dh, dw)
        skip = cur
        if dh or dw:
            if rng.random() < 0.5:
                up = net.crop(((0, dh), (dw, 0)), src=up)
            else:
                skip = net.zeropad2(((dh, 0), (0, dw)), src=cur)
        net.concat([up, skip] if rng.random() < 0.7 else [skip, up])
        return clipped(pick((16, 32)) if mfma else pick(small), a, a)

    def growth(cur):
        for _ in range(2):
            new = clipped(pick((5, 8, 12)), src=cur)
            cur = net.concat([cur, new])
        return clipped(pick(small), k=1)

    def inception(cur):
        outs = []
        for _ in range(int(rng.integers(2, 5))):
            b = pick(("1x1", "3x3", "pool", "dw")) if left[0] > 2 else "pool"
            if b == "1x1":
                outs.append(clipped(pick((3, 5, 8, 12)), k=1, src=cur))
            elif b == "3x3":
                outs.append(clipped(pick((8, 16, 24)), src=cur))
            elif b == "pool":
                outs.append(net.pool("maxpool", (3, 3), (1, 1), "same", src=cur))
            else:
                outs.append(depthwise(cur, s=1, a=pick(akeys)))
        net.concat(outs)
        return clipped(pick(small), k=1)

    stem_a = {"mfma": "q4", "pk16": "q4"}.get(force)
    cur = clipped(pick((8, 12, 16)) if force is None else 16, stem_a, stem_a)
    blocks = ([force] if force else []) + [pick(("group", "pool", "identity", "encdec", "encdec", "separable", "separable",
                                                 "growth", "inception")) for _ in range(int(rng.integers(2, 5)))]
    for block in blocks:
        h, w_, c = net.shape[cur]
        start = cur
        residual = block in ("separable", "inception", "encdec") and left[0] >= 5 and rng.random() < 0.3
        if block == "mfma":
            cur = encdec(cur, mfma=True)
        elif block == "pk16":
            cur = separable(cur, M=1, k=3, s=1, dil=1, w="q4", a="q4")
        elif block == "pool" and min(h, w_) >= 4:
            cur = net.pool("maxpool", pick(((2, 2), (3, 3), (2, 3))), pick(((2, 2), (1, 1))), pick(("same", "valid")))
        elif block == "identity" and left[0] >= 2:
            clipped(c, src=cur)
            left[0] -= 1
            net.conv(c, *WEIGHT_OF[pick(wkeys)])
            main = net.bn()
            net.add(cur, main)
            net.scale(0.5)
            cur = act()
        elif block == "encdec" and left[0] >= 3 and min(h, w_) >= 4:
            cur = encdec(cur)
        elif block == "separable" and left[0] >= 2:
            cur = separable(cur, s=1 if residual else None)
        elif block == "growth" and left[0] >= 3:
            cur = growth(cur)
        elif block == "inception" and left[0] >= 3:
            cur = inception(cur)
        elif left[0] >= 1:
            cur = clipped(pick(small))
        if residual and cur != start and net.shape[cur][:2] == net.shape[start][:2] and left[0] >= 1:
            left[0] -= 1
            net.conv(c, *WEIGHT_OF[pick(wkeys)], k=1)
            main = net.bn()
            net.add(start, main)
            net.scale(0.5)
            cur = act()
    h, w_, c = net.shape[cur]
    head = pick(("flat", "tail", "global"))
    if head == "flat":
        net.flatten()
    elif head == "tail":
        net.pool("avgpool", 8 if min(h, w_) >= 8 else 4 if min(h, w_) >= 4 else 2 if min(h, w_) >= 2 else 1)
        net.flatten()
    else:
        net.pool("globalmaxpool")
    net.dense(10, *WEIGHT_OF[pick(wkeys)], bias=bool(head != "tail" and rng.random() < 0.5))
    if rng.random() < 0.25:
        net.softmax()
    assert left[0] >= 0, left
    x = (rng.integers(0, 9, (N, net.hw[0], net.hw[1], 3)) / 8.0).astype(F32)
    return net.spec, x, net.shape["input"]


# ---- what the wide lists must cover ----------------------------------------------------------------------------------------
def categories_wide(spec, image=(8, 8, 3)):
    c = categories(spec) | plan(spec, image)[2]
    ops = {op["op"] for op in spec}
    if any(op["op"] == "zeropad" and spatial_desc(op) is not None for op in spec):
        c.add("op zeropad (pair form)")
    new = ops & {"concat", "crop", "upsample", "dwconv", "tconv"} or "op zeropad (pair form)" in c
    if new and "concat" not in ops and not any(op["op"] in ("conv", "dense") and op["kind"] == "float" for op in spec):
        c.add("LayerModel chain")
    return c


REQUIRED_OLD = frozenset(REQUIRED)
REQUIRED_WIDE = (
    {"op %s" % k for k in ("concat", "crop", "upsample", "zeropad (pair form)", "dwconv", "tconv")} |
    {"codes through %s: %s" % (o, s) for o in ("crop", "upsample", "zeropad", "concat") for s in ("bin", "i4", "i8", "t2")
     if (o, s) != ("zeropad", "bin")} |                       # a +-1 code has no zero
    {"%s codes through a spatial op or concat" % k for k in ("relu", "leaky", "2-bit", "3-bit")} |
    {"concat join: codes", "concat join: clips", "concat join: float32", "pack_clips join",
     "packed producer, other store wanted", "dwconv clip in the epilogue", "tconv clip in the epilogue",
     "BN behind dwconv read twice", "BN behind tconv read twice", "ternary: no common store behind a concat",
     "tconv matrix-pipe form", "depthwise 16-bit-lane form", "LayerModel chain"} |
    {"max activation in front of %s" % k for k in ("dwconv", "tconv", "spatial", "concat")})
REQUIRED = REQUIRED | REQUIRED_WIDE


# ============================================================================================================================
# The grouped convolution: {"op": "gconv"} (Net.gconv) in the reference, the guard and plan() above.
#
#   HAND_GROUPED              one spec per planner decision about a gconv, the pivotal ones with the log written out
#   generate_grouped(seed)    random ResNeXt / ShuffleNet-style networks
#   categories_grouped(spec)  categories_wide plus the gconv launch names; REQUIRED_GROUPED is what the two lists must cover
# ============================================================================================================================
HAND_GROUPED = []


def _grouped(name, net, log=None, layer_model=None, same_scaled_log=False):
    """As _wide.  same_scaled_log: GraphModel(scaled_codes=True) must log what GraphModel() logs although the spec holds a
    batch-maximum activation."""
    assert name not in [c["name"] for c in HAND_GROUPED], name
    HAND_GROUPED.append(dict(name=name, spec=net.spec, x=net.images(), image=net.shape["input"], log=log,
                             layer_model=layer_model, same_scaled_log=same_scaled_log))


def _gstem(name, c=8, w="q4", a="q4", hw=(8, 8)):
    net = Net(_seed("grouped_" + name), hw=hw)
    net.clipped(c, w, a, dst="a0")
    return net


def _gclip(net, cout, w="q4", a="q4", groups=2, bn=True, dst=None, **kw):
    """gconv -> [bn] -> clip; `a`: a key of ACT_OF or (fn, bits)."""
    net.gconv(cout, *WEIGHT_OF[w], groups=groups, bias=kw.pop("bias", True), **kw)
    if bn:
        net.bn()
    return net.act(*(ACT_OF[a] if isinstance(a, str) else a), dst=dst)


_SNAME = {"q4": "i4", "q8": "i8", "bin": "bin", "tern": "t2"}

# -- the ResNeXt bottleneck 1x1 -> gconv -> 1x1 with an identity add, on the matrix pipe: Fg < 16 with t > 1 (Cg = Fg = 4,
#    g = 4) and Fg = 16 (g = 2 of 32), int4 and int8
for _a, _c, _g in (("q4", 16, 4), ("q8", 32, 2), ("q4", 32, 2), ("q8", 16, 4)):
    for _add in (True, False):
        _n = "bottleneck_%s_c%d_g%d%s" % (_a, _c, _g, "" if _add else "_no_add")
        if not _add and (_a, _c) not in (("q4", 16), ("q8", 32)):
            continue
        net = _gstem(_n, _c, _a, _a)
        net.clipped(_c, _a, _a, k=1)
        _gclip(net, _c, _a, _a, _g)
        net.conv(_c, *WEIGHT_OF[_a], k=1)
        main = net.bn()
        if _add:
            net.add("a0", main)
            net.scale(0.5)
        net.act(*ACT_OF[_a])
        _head(net, _a)
        _grouped(_n, net, log=["pack", "gconv_%s_mfma" % _SNAME[_a]])

# -- the plain form by shape: 12 -> 12 in three groups, and group edges inside input words (Cg of 5, 3, 33)
for _n, _w, _cin, _cout, _g, _k in (("12_g3", "q4", 12, 12, 3, "gconv_i4_plain"), ("i4_cg5", "q4", 10, 6, 2, "gconv_i4_plain"),
                                    ("i8_cg3", "q8", 12, 8, 4, "gconv_i8_plain"), ("bin_cg5", "bin", 10, 6, 2, "gconv_bin"),
                                    ("bin_cg33", "bin", 66, 10, 2, "gconv_bin"), ("t2_cg33", "tern", 66, 10, 2, "gconv_t2")):
    _a = _w
    net = _gstem("plain_" + _n, _cin, _w, _a, hw=(9, 7))
    _gclip(net, _cout, _w, _a, _g)
    net.clipped(8, _w, _a)
    _head(net, _w)
    _grouped("plain_by_shape_" + _n, net, log=["pack", _k])

# -- the plain form by epilogue on a matrix-pipe shape (16 -> 16, g = 4): q4 codes in, an 8-bit clip, no clip, a 1-bit clip
for _n, _a in (("q8_clip", "q8"), ("binary_clip", "bin")):
    net = _gstem("epi_" + _n, 16)
    _gclip(net, 16, "q4", _a, 4)
    net.clipped(8, "q8" if _a == "q8" else "bin", "q4")
    _head(net)
    _grouped("plain_by_epilogue_" + _n, net, log=["pack", "gconv_i4_plain"])
net = _gstem("epi_none", 16)
net.gconv(16, groups=4, bias=True)
b = net.bn()
net.add("a0", b)
net.scale(0.5)
net.act()
_head(net)
_grouped("plain_by_epilogue_no_clip", net, log=["pack", "gconv_i4_plain"])

# -- every clip function at 2, 3, 4 and 8 bits in the epilogue (and binary_tanh), read by a conv of the matching store
for _fn in ("quantized_tanh", "quantized_relu", "quantized_leakyrelu"):
    for _nb in (2, 3, 4, 8):
        _n = "epilogue_%s_%d" % (_fn, _nb)
        net = _gstem(_n, 8, hw=(9, 7) if _nb in (3, 8) else (8, 8))
        _gclip(net, 8, "q4", (_fn, _nb), 2, bn=_nb != 3)
        net.clipped(8, "q8" if _nb == 8 else "q4", "q4")
        _head(net)
        _grouped(_n, net)
net = _gstem("epilogue_bin", 8, "bin", "bin")
_gclip(net, 8, "bin", "bin", 4)
net.clipped(8, "bin", "bin")
_head(net, "bin")
_grouped("epilogue_binary_tanh", net, log=["pack", "gconv_bin"])

# -- BN absent, BN read twice, a second reader beside the BN, the clip read twice, the packed output as the last tensor
net = _gstem("no_bn")
_gclip(net, 8, bn=False)
net.clipped(8)
_head(net)
_grouped("gconv_without_bn", net, log=["pack", "gconv_i4_plain"])
net = _gstem("bn_twice")
net.gconv(8, groups=2, bias=True)
b = net.bn(dst="b")
a1 = net.act(src=b, dst="a1")
net.clipped(8, src=a1, dst="a2")
net.act("quantized_tanh", 8, src=b, dst="a3")
net.concat(["a2", "a3"])
net.clipped(8)
_head(net)
_grouped("gconv_bn_read_twice", net, log=["pack", "gconv_i4_plain", "concat_f32"])
net = _gstem("beside_bn")
y = net.gconv(8, groups=2, bias=True, dst="y")
net.bn()
a1 = net.act(dst="a1")
net.act("quantized_relu", 4, src=y, dst="a2")
net.clipped(8, src=a1, dst="c1")
net.clipped(8, src="a2", dst="c2")
net.add("c1", "c2")
net.act()
_head(net)
_grouped("gconv_second_reader_beside_bn", net, log=["pack", "gconv_i4_plain"])
net = _gstem("clip_twice")
y = _gclip(net, 8)
net.pool("maxpool", (2, 2), (2, 2), "valid", src=y, dst="p")
net.clipped(8, s=2, src=y, dst="c")
net.concat(["p", "c"])
net.clipped(8)
_head(net)
_grouped("gconv_clip_read_twice", net)
net = _gstem("last")
_gclip(net, 8, a="leaky4")
_grouped("gconv_clip_is_last", net, log=["pack", "gconv_i4_plain"])

# -- who reads the packed output: (conv: above) dense behind flatten, dwconv, tconv, another gconv, add, the new-form pools,
#    crop / upsample / pair zeropad, concat
net = _gstem("r_flat", hw=(4, 4))
_gclip(net, 8)
_head(net)
_grouped("gconv_then_flatten_dense", net)
net = _gstem("r_dw")
_gclip(net, 8)
net.dwconv(1, bias=True)
net.bn()
net.act()
net.clipped(8, k=1)
_head(net)
_grouped("gconv_then_dwconv", net, log=["pack", "gconv_i4_plain", "depthwise_i4"])
net = _gstem("r_tc", hw=(4, 4))
_gclip(net, 8)
net.tconv(8, k=2, s=2, bias=True)
net.bn()
net.act()
net.clipped(8)
_head(net, flat=False)
_grouped("gconv_then_tconv", net, log=["pack", "gconv_i4_plain", "tconv_i4_plain", "pool_max_i4"])
net = _gstem("r_gc", 16)
_gclip(net, 16, groups=4)
_gclip(net, 12, groups=2)
net.clipped(8)
_head(net)
_grouped("gconv_then_gconv", net, log=["pack", "gconv_i4_mfma", "gconv_i4_plain"])
net = _gstem("r_add")
y = _gclip(net, 8)
net.add("a0", y)
net.scale(0.5)
net.act()
_head(net)
_grouped("gconv_then_add", net)
net = _gstem("r_maxpool", hw=(9, 7))
_gclip(net, 8)
net.pool("maxpool", (3, 3), (2, 2), "same")
net.clipped(8)
_head(net)
_grouped("gconv_then_new_maxpool", net, log=["pack", "gconv_i4_plain", "pool_max_i4"])
net = _gstem("r_avgpool")
_gclip(net, 8)
net.pool("avgpool", (2, 2), (2, 2), "valid")
_head(net)
_grouped("gconv_then_new_avgpool", net, log=["pack", "gconv_i4_plain", "pool_avg_i4"])
net = _gstem("r_gpool", a="q8", w="q8")
_gclip(net, 8, "q8", "q8")
_head(net, "q8", flat=False)
_grouped("gconv_then_global_maxpool", net, log=["pack", "gconv_i8_plain", "pool_max_i8"])
net = _gstem("r_spatial", hw=(9, 7))
_gclip(net, 8, a="relu4")
net.crop(((0, 1), (1, 0)))
net.upsample((1, 2))
net.clipped(8)
_head(net)
_grouped("gconv_then_crop_upsample", net, log=["pack", "gconv_i4_plain", "spatial_i4", "spatial_i4"])
net = _gstem("r_up")
_gclip(net, 8, a="q2", w="q2")
net.upsample((2, 1))
net.clipped(8, s=2)
_head(net)
_grouped("gconv_then_upsample", net)
net = _gstem("r_pad", hw=(9, 7))
_gclip(net, 8, a="q3")
net.zeropad2(((1, 0), (0, 2)))
net.clipped(8, pad="valid")
_head(net)
_grouped("gconv_then_pair_zeropad", net, log=["pack", "gconv_i4_plain", "spatial_i4"])

# -- the join with the skip (the `upsampled` set of forward: the concat packs the skip to meet the gconv's codes): the skip
#    first and second, int4, int8 and 1-bit codes
for _a, _c, _g in (("q4", 16, 4), ("q8", 16, 4), ("bin", 12, 3), ("q4", 12, 3)):
    for _first in (False, True):
        _n = "join_%s_c%d_skip_%s" % (_a, _c, "first" if _first else "second")
        net = _gstem(_n, _c, _a, _a, hw=(9, 7) if _first else (8, 8))
        _gclip(net, _c, _a, _a, _g, dst="b")
        net.concat(["a0", "b"] if _first else ["b", "a0"])
        net.clipped(16, _a, _a, k=1)
        _head(net, _a)
        _s = _SNAME[_a]
        _k = "gconv_" + (_s if _a == "bin" else _s + ("_mfma" if _c == 16 else "_plain"))
        _grouped(_n, net, log=["pack", _k, "concat_" + _s])
# a skip of another width: the codes meet a clip they cannot be joined with, the join runs in float32
net = _gstem("join_width", 16)
_gclip(net, 16, "q4", "q2", 4, dst="b")
net.concat(["b", "a0"])
net.clipped(8)
_head(net)
_grouped("join_skip_of_another_width", net, log=["pack", "gconv_i4_mfma", "concat_f32"])
# a ternary gconv on grid codes; its ternary activation travels as planes and meets the ternary skip as planes
net = _gstem("join_tern", 8, "tern", "tern")
net.gconv(8, "ternary", 1, groups=2, bias=True, src="a0")
net.bn()
net.act("ternary_tanh", dst="t")
net.upsample((1, 1), dst="u")
net.concat(["u", "a0"], dst="cat")
net.gconv(8, "ternary", 1, groups=4, k=(2, 3))
net.bn()
net.act("ternary_tanh")
_head(net, "tern")
_grouped("join_ternary_planes", net, log=["pack", "gconv_t2", "spatial_t2", "concat_t2", "gconv_t2"])

# -- weight kinds on q4 codes, the re-clip branch (a packed producer of another store), grid codes read by binary weights
for _w in ("bin", "tern", "q2", "q3", "q8"):
    net = _gstem("w_" + _w, 12, hw=(9, 7))
    _gclip(net, 8, _w, "q4", 4)
    net.clipped(8)
    _head(net)
    _grouped("weights_%s_on_q4_codes" % _w, net, log=["pack", "gconv_i8_plain" if _w == "q8" else "gconv_i4_plain"])
net = _gstem("reclip", 8)
_gclip(net, 8, "q4", "bin", 2)                                        # 1-bit codes ...
_gclip(net, 8, "q8", "q8", 2)                                         # ... read by 8-bit weights: another store
_head(net, "q8")
_grouped("gconv_other_store_wanted", net, log=["pack", "gconv_i4_plain", "pack", "gconv_i8_plain"])
net = _gstem("grid_bin", 10, "tern", "tern")
_gclip(net, 6, "bin", "bin", 2)
net.clipped(8, "bin", "bin")
_head(net, "bin")
_grouped("binary_gconv_on_grid_codes", net, log=["pack", "gconv_i4_plain"])
# float weights: behind a clip, and behind a packed tensor (read as float32 without an `unpack` launch)
net = _gstem("float_clip")
net.gconv(8, "float", 0, groups=2, s=2, pad="valid", bias="dyadic")
net.act()
net.clipped(8)
_head(net)
_grouped("float_gconv_behind_a_clip", net, log=["gconv_f32"])
net = _gstem("float_packed")
net.pool("maxpool", (2, 2), (2, 2), "valid")
net.gconv(8, "float", 0, groups=4, bias="dyadic")
net.bn()
net.act()
_head(net)
_grouped("float_gconv_behind_packed_codes", net, log=["pool_max_i4", "gconv_f32"])

# -- geometry on the 9 x 7 maps: stride 2 ('same' and 'valid'), dilation 2, windows 1 x 1, 5 x 5, 2 x 3
for _n, _kw in (("s2_same", dict(s=2)), ("s2_valid", dict(s=2, pad="valid")), ("dil2", dict(dil=2)), ("k1", dict(k=1)),
                ("k5", dict(k=5)), ("k2x3", dict(k=(2, 3), pad="valid")), ("k5_dil2_mfma", dict(k=5, dil=(1, 2)))):
    _mf = _n.endswith("mfma")
    net = _gstem("geom_" + _n, 16 if _mf else 12, hw=(9, 7))
    _gclip(net, 16 if _mf else 12, groups=4 if _mf else 3, **_kw)
    net.clipped(8)
    _head(net)
    _grouped("geometry_" + _n, net, log=["pack", "gconv_i4_mfma" if _mf else "gconv_i4_plain"])

# -- a gconv as the first layer, on the images: g = 3 and g = 1 with low-bit weights, float weights
for _n, _w, _g, _c in (("g3_q4", "q4", 3, 6), ("g1_bin", "bin", 1, 8), ("g3_tern", "tern", 3, 12)):
    net = Net(_seed("first_" + _n), hw=(8, 8))
    _gclip(net, _c, _w, "q4", _g)
    net.clipped(8)
    _head(net)
    _grouped("first_layer_" + _n, net, log=["gconv_f32"])
net = Net(_seed("first_float"), hw=(9, 7))
net.gconv(6, "float", 0, groups=3, bias="dyadic")
net.act()
net.clipped(8)
_head(net)
_grouped("first_layer_float", net, log=["gconv_f32"])

# -- a batch-maximum activation in front: read as float32, with and without scaled codes
net = Net(_seed("grouped_max"), hw=(8, 8))
net.conv(8, bias=True)
net.act("quantized_maxrelu", 4)
_gclip(net, 8)
net.clipped(8)
_head(net)
_grouped("gconv_behind_max_activation", net, log=["gconv_f32"], same_scaled_log=True)

# -- groups = 1 and groups = Cin (test_spec_graph_cpu.py: the reference equals that of the conv / dwconv twin)
for _n, _w, _a in (("q4", "q4", "q4"), ("tern", "tern", "tern"), ("bin", "bin", "bin")):
    net = _gstem("g1_" + _n, 8, _w, _a, hw=(9, 7))
    _gclip(net, 12, _w, _a, 1, s=2)
    net.clipped(8, _w, _a)
    _head(net, _w)
    _grouped("groups_1_" + _n, net)
    net = _gstem("gcin_" + _n, 8, _w, _a, hw=(9, 7))
    _gclip(net, 16, _w, _a, 8, dil=2)
    net.clipped(8, _w, _a)
    _head(net, _w)
    _grouped("groups_cin_" + _n, net)
GROUPS_ONE = tuple("groups_1_" + n for n in ("q4", "tern", "bin"))
GROUPS_CIN = tuple("groups_cin_" + n for n in ("q4", "tern", "bin"))

CAPTURED_GROUPED = ("bottleneck_q4_c16_g4", "join_q4_c16_skip_second")


def conv_twin(spec):
    """The spec with every gconv of groups = 1 written as a conv."""
    out = []
    for op in spec:
        if op["op"] == "gconv":
            assert op["groups"] == 1
            op = {k: v for k, v in op.items() if k not in ("groups", "dilation", "H")}
            op.update(op="conv", dilation_rate=dw_dilation(spec[len(out)]))
        out.append(op)
    return out


def dwconv_twin(spec):
    """The spec with every gconv of groups = Cin written as a dwconv: M = Fg, kernel (kh, kw, 1, C * M) -> (kh, kw, C, M)."""
    out = []
    for op in spec:
        if op["op"] == "gconv":
            kh, kw, cg, cout = op["kernel"].shape
            assert cg == 1 and cout % op["groups"] == 0
            M = cout // op["groups"]
            op = {k: v for k, v in op.items() if k != "groups"}
            op.update(op="dwconv", kernel=op["kernel"].reshape(kh, kw, cout // M, M), depth_multiplier=M)
        out.append(op)
    return out


# ---- the third generator -----------------------------------------------------------------------------------------------------
SEEDS_GROUPED = range(32)
GROUPED_BASE = 110000
WKEYS_WIDE = ("bin", "tern", "q2", "q3", "q4", "q4", "q8")                # generate_wide's key lists
AKEYS_WIDE = ("bin", "q2", "q3", "q4", "q4", "q8", "relu4", "relu8", "leaky4", "leaky2", "tern")


def _divisors(cin, cout):
    return [d for d in range(1, cin + 1) if cin % d == 0 and cout % d == 0]


def generate_grouped(seed):
    """(spec, images, image shape) of a random network around grouped convolutions: a stem, 2 to 4 blocks out of {ResNeXt
    bottleneck with or without the add, ShuffleNet-style branch concatenated with its skip, grouped stem, gconv -> new-form
    pool, inception branches with a gconv beside a dwconv, plain group} and a head of generate_wide; `groups` is drawn from
    the common divisors of the two channel counts, weights and activations per op.  Seeds 0 mod 4 hold a matrix-pipe
    gconv (16 or 32 channels, q4 or q8 throughout), seeds 1 mod 4 a plain-form gconv on packed input."""
    rng = np.random.default_rng(GROUPED_BASE + seed)
    force = {0: "mfma", 1: "plain"}.get(seed % 4)
    net = Net(GROUPED_BASE + 10000 + seed, hw=(8, 8) if rng.random() < 0.5 else (9, 7))
    pick = lambda seq: seq[int(rng.integers(len(seq)))]      # noqa: E731
    use_max = force is None and rng.random() < 0.25
    through = pick(("q4", "q8")) if force == "mfma" else None
    left = [MAX_CONTRACTIONS_WIDE - 1]                       # (the head's dense is one)
    small = tuple(c for c in CHANNELS_WIDE if c <= 33)
    last_a = [None]

    def act(a=None):
        if a is None and use_max and rng.random() < 0.4:
            last_a[0] = None
            return net.act(pick(("quantized_maxrelu", "quantized_leakymaxrelu")), pick((3, 4)))
        last_a[0] = a or through or pick(AKEYS_WIDE)
        return net.act(*ACT_OF[last_a[0]])

    def clipped(cout, w=None, a=None, **kw):
        left[0] -= 1
        net.conv(cout, *WEIGHT_OF[w or through or pick(WKEYS_WIDE)], bias=bool(rng.random() < 0.5), **kw)
        if rng.random() < 0.8:
            net.bn()
        return act(a)

    def grouped(cout, src=None, g=None, w=None, a=None, clip=None, free=False):
        """gconv -> [bn] -> [clip]; free: window, stride, dilation and padding are drawn too."""
        left[0] -= 1
        h, w_, cin = net.shape[net.cur if src is None else src]
        k, s, dil, pad = 3, 1, 1, "same"
        if free:
            k, s, pad = pick((3, 3, 1, (2, 3), 5)), pick((1, 1, 2)), pick(("same", "same", "valid"))
            dil = pick((1, 1, 2)) if s == 1 and k != 1 else 1
            if pad == "valid" and min(h, w_) < D.effective(max(P.pair(k)), dil):
                pad = "same"
        clip = (a is not None or rng.random() < 0.85) if clip is None else clip
        net.gconv(cout, *WEIGHT_OF[w or through or pick(WKEYS_WIDE)], groups=pick(_divisors(cin, cout)) if g is None else g, k=k,
                  s=s, dil=dil, pad=pad, bias=(bool(rng.random() < 0.5) if clip else "dyadic"), src=src)
        if rng.random() < 0.7:
            net.bn() if clip else net.dyadic_bn()
        return act(a) if clip else net.cur

    def bottleneck(cur, mfma=False):
        c = net.shape[cur][2]
        mid = pick((16, 32)) if mfma else pick((8, 12, 16, 24, 32))
        clipped(mid, k=1, src=cur)
        g = pick([d for d in _divisors(mid, mid) if GC.plan(3, 3, mid, mid, d) is not None]) if mfma else None
        grouped(mid, g=g, a=through, clip=True if mfma else None)
        left[0] -= 1
        net.conv(c, *WEIGHT_OF[through or pick(WKEYS_WIDE)], k=1)
        main = net.bn()
        if rng.random() < 0.6:
            net.add(cur, main) if rng.random() < 0.5 else net.add(main, cur)
            net.scale(0.5)
        return act()

    def shuffle(cur):
        c, skip_a = net.shape[cur][2], last_a[0]
        src = cur
        if left[0] >= 4 and rng.random() < 0.4:
            src = clipped(pick((8, 12, 16)), k=1, src=cur)
        b = grouped(pick((8, 12, 16, c)), src=src, a=skip_a if rng.random() < 0.6 else None, clip=True)
        net.concat([b, cur] if rng.random() < 0.5 else [cur, b])
        return clipped(pick(small), k=1)

    def inception(cur):
        outs = [grouped(pick((8, 12, 16)), src=cur, clip=True)]
        left[0] -= 1
        net.dwconv(1, *WEIGHT_OF[pick(WKEYS_WIDE)], bias=bool(rng.random() < 0.5), src=cur)
        net.bn()
        outs.append(act())
        if rng.random() < 0.5:
            outs.append(net.pool("maxpool", (3, 3), (1, 1), "same", src=cur))
        net.concat(outs)
        return clipped(pick(small), k=1)

    if force == "plain":
        cur = clipped(pick((12, 16)), "q4", "q4")
    else:
        cur = clipped(pick((16, 32)) if force else pick((8, 12, 16)), through, through)
    blocks = ([force] if force else []) + [pick(("bottleneck", "bottleneck", "shuffle", "shuffle", "gstem", "gpool", "inception",
                                                 "group")) for _ in range(int(rng.integers(2, 5)))]
    for block in blocks:
        h, w_, c = net.shape[cur]
        if block == "mfma":
            cur = bottleneck(cur, mfma=True)
        elif block == "plain":                               # by shape (12 in 3 groups) or by epilogue (16 in 4, an 8-bit clip)
            cur = grouped(c, src=cur, g=3 if c == 12 else 4, w="q4", a="q4" if c == 12 else "q8")
        elif block == "bottleneck" and left[0] >= 3:
            cur = bottleneck(cur)
        elif block == "shuffle" and left[0] >= 2:
            cur = shuffle(cur)
        elif block == "gpool" and left[0] >= 1 and min(h, w_) >= 4:
            grouped(pick(small), src=cur, clip=True)
            cur = net.pool("maxpool", pick(((2, 2), (3, 3), (2, 3))), pick(((2, 2), (1, 1))), pick(("same", "valid")))
        elif block == "inception" and left[0] >= 3:
            cur = inception(cur)
        elif block == "group" and left[0] >= 1:
            cur = clipped(pick(small))
        elif left[0] >= 1:                                   # the grouped stem (and whatever found no room)
            cur = grouped(pick(small), src=cur, free=True)
    h, w_, c = net.shape[cur]
    head = pick(("flat", "tail", "global"))
    if head == "flat":
        net.flatten()
    elif head == "tail":
        net.pool("avgpool", 8 if min(h, w_) >= 8 else 4 if min(h, w_) >= 4 else 2 if min(h, w_) >= 2 else 1)
        net.flatten()
    else:
        net.pool("globalmaxpool")
    net.dense(10, *WEIGHT_OF[through or pick(WKEYS_WIDE)], bias=bool(head != "tail" and rng.random() < 0.5))
    if rng.random() < 0.25:
        net.softmax()
    assert left[0] >= 0, left
    x = (rng.integers(0, 9, (N, net.hw[0], net.hw[1], 3)) / 8.0).astype(F32)
    return net.spec, x, net.shape["input"]


# ---- what the grouped lists must cover -------------------------------------------------------------------------------------
GCONV_LAUNCHES = ("gconv_f32", "gconv_bin", "gconv_t2", "gconv_i4_mfma", "gconv_i4_plain", "gconv_i8_mfma", "gconv_i8_plain")
GCONV_READERS = ("conv", "flatten", "dwconv", "tconv", "gconv", "add", "maxpool (new form)", "avgpool (new form)",
                 "globalmaxpool", "crop", "upsample", "zeropad", "concat")


def categories_grouped(spec, image=(8, 8, 3)):
    c = categories_wide(spec, image)
    c |= {"launch %s" % k for k in plan(spec, image)[1] if k.startswith("gconv_")}
    if any(op["op"] == "gconv" for op in spec) and not any(op["op"] == "concat" for op in spec) and \
            not any(op["op"] in ("conv", "dense") and op["kind"] == "float" for op in spec):
        c.add("LayerModel chain")
    return c


REQUIRED_GROUPED = (
    {"op gconv", "gconv clip in the epilogue", "BN behind gconv read twice", "a second reader beside the BN behind gconv",
     "clip behind gconv read twice", "packed gconv output is the last tensor", "gconv matrix-pipe form",
     "gconv plain form: other out store", "packed producer, other store wanted", "pack_clips join",
     "concat: codes meet a clip, joined in float32", "max activation in front of gconv", "LayerModel chain"} |
    {"launch %s" % k for k in GCONV_LAUNCHES} | {"packed gconv output read by %s" % k for k in GCONV_READERS})
