"""Whole-network runners over a net spec (nets.py): the only way from a spec to the HIP library.

  FusedModel          chains (VGG): every conv -> BN -> activation clip -> max-pool group is ONE kernel launch whose
                      epilogue writes the next layer's input already packed at the activation width ("M1" traffic
                      model); inter-layer tensors never exist in float32.  What nets.Model runs for a
                      chain, and what bench.py times step by step (steps / run_step / bind).
  ResidualFusedModel  every other topology (ResNet): the same fusion plus the residual merge
                      conv -> BN -> add(shortcut) -> [x0.5] -> act in one launch, evaluated on demand from the output,
                      and the classifier tail avg-pool -> Flatten -> Dense -> softmax behind a packed activation in one
                      launch; what is on neither path runs as float32 torch ops.  What
                      nets.Model runs for everything FusedModel refuses (NotFusable).
  Pipelined           a fused engine's forward with several batches in flight: bound launch plans (FusedModel.bind) or
                      hipGraphs of model(x) per lane.  What nets.Model.predict and bench.py's timed region run.
  GraphModel          general interpreter, one launch per contraction with the activation clip fused into its
                      pack-on-load and BN into its epilogue; the stock Keras layers around it are float32 torch ops.
                      The plain counterpart the tests hold the fused engines against, and the one engine that runs
                      {"op": "merge", "fn": "add|sub|mul|avg|max|min", "srcs": [...]} (Keras' element-wise merge layers,
                      qnn_merge_forward: on the codes where every branch hands codes of one store and width) and
                      {"op": "concat", "srcs": [...]} (channel concatenation, qnn_concat_forward: on packed codes
                      where every branch hands codes of one store) and the new-form spatial ops {"op": "crop"},
                      {"op": "upsample"} and {"op": "zeropad", "pad": ((t, b), (l, r))} (qnn_spatial2d_forward: behind
                      a low-bit clip the codes are moved and stay packed); nets.Model falls to it for such a spec.
                      Also the one fused home of {"op": "dwconv"} (depthwise convolution, qnn_depthwise_forward): a
                      following bn and low-bit activation go into its epilogue and a packed producer into its input, so
                      pack -> dwconv -> 1x1 conv keeps codes throughout.  {"op": "tconv"} (transposed convolution,
                      qnn_tconv_forward) runs under the same rules; the codes it leaves meet a skip as codes in a concat.
                      {"op": "gconv"} (grouped convolution, qnn_gconv_forward) runs under the rules of tconv: its codes
                      meet a skip as codes in a concat too.
  LayerModel          the Keras-compatible layer objects called one by one (float32 NHWC in, float32 NHWC out per
                      layer: "M0" traffic model); nets.Model.conv_output reads intermediate tensors through it.

The three spec interpreters share one reading of the spec (_SpecGraph) and one set of float32 glue ops (_GLUE); the two
fused engines share the "auto" first-layer protocol (_DomainFlag).  All engines produce identical logits; tests compare
them with the CPU oracle.  None of them has a CPU path.
"""
import contextlib
import math

import numpy as np
import torch

from . import _abi
from .layers.binary_layers import BinaryConv2D, BinaryDense
from .layers.quantized_layers import QuantizedConv2D, QuantizedDense
from .layers.ternary_layers import TernaryConv2D, TernaryDense
from .layers.depthwise import (DepthwiseConv2D, BinaryDepthwiseConv2D, QuantizedDepthwiseConv2D,
                               TernaryDepthwiseConv2D)
from .layers.conv_transpose import (Conv2DTranspose, BinaryConv2DTranspose, QuantizedConv2DTranspose,
                                    TernaryConv2DTranspose)
from .layers.grouped import GroupedConv2D, BinaryGroupedConv2D, QuantizedGroupedConv2D, TernaryGroupedConv2D
from .layers import binary_ops, quantized_ops, ternary_ops

F32 = np.float32

# Ternary activations x ternary weights (full-tnn networks, layers/ternary_layers.py) are stored as sign / mask bit
# planes (QNN_STORE_T2, 2 bits per value) and contracted with two popcounts.  False = keep them as int4 codes (the
# round-2 form; bit-identical results, tests run both).
TERNARY_T2 = True


def bn_constants(op):
    """tf.nn.batch_normalization constants in float32, formed on the host exactly
    as the oracle does: inv = (1/sqrt(var+eps))*gamma; shift = beta - mean*inv."""
    gamma, beta, mean, var = (np.asarray(op[k], dtype=F32) for k in ("gamma", "beta", "mean", "var"))
    inv = (F32(1) / np.sqrt(var + F32(op["eps"]))).astype(F32) * gamma
    shift = beta - mean * inv
    return inv.astype(F32), shift.astype(F32)


def _wkind(op):
    return {"binary": _abi.W_BINARY, "quantized": _abi.W_QUANT, "float": _abi.W_FLOAT,
            "ternary": _abi.W_TERNARY}[op["kind"]]


def _wstore(op):
    """Narrowest packed storage of a contraction's weights (None for float)."""
    if op["kind"] == "binary":
        return _abi.STORE_BIN
    if op["kind"] == "ternary":
        return _abi.STORE_I4                 # codes {-1, 0, 1}
    if op["kind"] == "quantized" and op["nb"] <= 8:
        return _abi.store_for_bits(op["nb"])
    return None


def _act_code(act):
    """(fn, bits) of an activation op, or None if it is not a low-bit clip.  None for quantized_maxrelu /
    quantized_leakymaxrelu too: their values P k / m follow the batch maximum and are not on the fixed grid k / m, so
    the activation is materialised as float32 and its consumers take the float-input kernels."""
    if act is None:
        return None
    if act["fn"] == "quantized_leakymaxrelu":
        quantized_ops.check_leaky_alpha(act.get("alpha", quantized_ops.LEAKY_ALPHA), "quantized_leakymaxrelu")
    if act["fn"] == "binary_tanh":
        return _abi.FN_BINARY_TANH, 1
    if act["fn"] in _QUANT_ACTS and act["nb"] <= 8:
        if act["fn"] == "quantized_leakyrelu":
            quantized_ops.check_leaky_alpha(act.get("alpha", quantized_ops.LEAKY_ALPHA))
        return _QUANT_ACTS[act["fn"]], int(act["nb"])
    return None


# the quantised activations of layers/quantized_ops.py: spec name -> QNN_FN_* (all three leave codes on the grid k / 2^(nb-1))
_QUANT_ACTS = {"quantized_tanh": _abi.FN_QUANTIZED_TANH, "quantized_relu": _abi.FN_QUANTIZED_RELU,
               "quantized_leakyrelu": _abi.FN_QUANTIZED_LEAKYRELU}
_NEW_QUANT_FNS = (_abi.FN_QUANTIZED_RELU, _abi.FN_QUANTIZED_LEAKYRELU)
# scaled by the maximum of the whole batch tensor (include/qnn_abi_maxact.h): elementwise ops on float32 only
_MAX_ACTS = ("quantized_maxrelu", "quantized_leakymaxrelu")


def scaled_route_exact(K, nb, wbits):
    """The exactness rule of the scaled route (include/qnn_abi_scaled.h).  A batch-scaled activation's consumer
    may read packed codes plus the device-resident scale instead of the float32 tensor only where the two routes give the
    same bits: the float32 route's fmaf chain over K products of an nb-bit activation code and a wbits-bit weight code
    (wbits = 1 for binary and ternary weights) is exact, and so equal to the integer sum, when every partial sum fits 24
    bits: K * 2^(nb-1) * 2^(wbits-1) <= 2^24.  4/4 networks qualify everywhere, 8/8 up to K = 1024."""
    return int(K) * 2 ** (int(nb) - 1) * 2 ** (int(wbits) - 1) <= 2 ** 24


def _scaled_route_pays(op, store):
    """False for the one family of consumers the scaled route would slow down (profiles/scaled/README.md, table b): a
    convolution the float32 route runs on the f32 matrix pipe (k_conv_f32act: 16 / 32 / 64 input channels, 3x3 at stride 1
    or 2 or 1x1 at stride 2, 'same', up to 256 filters in multiples of 16, undilated -- f32act_shape of csrc/qnn_f32act.hip)
    while its scaled call would find no matrix-pipe kernel (qnn_route_gemm's scaled tiles need 64 input channels and a
    multiple of 128 filters) and fall to k_conv_generic.  Such a consumer keeps the float32 tensor."""
    if op["op"] != "conv":
        return True
    kh, kw, cin, cout = op["kernel"].shape
    stride = tuple(op.get("strides", (1, 1)))[0]
    f32act = cin in (16, 32, 64) and cout % 16 == 0 and cout <= 256 and op.get("padding", "same") == "same" and kh == kw and \
        ((kh == 3 and stride in (1, 2)) or (kh == 1 and stride == 2)) and _dilation(op) == (1, 1)
    tiles = cin % 64 == 0 and cout % 128 == 0 and store in (_abi.STORE_I4, _abi.STORE_I8) and kh * kw <= 9
    return tiles or not f32act


def _refuse_max_acts(spec, who):
    """The packed engines carry codes on the fixed grid k / 2^(nb-1); an activation whose scale is the batch maximum has
    no such codes (packed codes plus a device-resident scale exist in GraphModel only, `scaled_codes`): GraphModel runs
    such a spec."""
    for op in spec:
        if op["op"] == "act" and op["fn"] in _MAX_ACTS:
            raise _abi.NotFusable("%s: activation %r scales by the maximum of the whole batch tensor; its values are not on "
                                  "the fixed grid k / 2^(nb-1) the packed kernels carry, so it cannot be fused into an "
                                  "epilogue or packed on load; use GraphModel" % (who, op["fn"]))


def _float_images(x, fn):
    """uint8 images in front of a layer whose epilogue is quantized_relu / quantized_leakyrelu: the QNN_STORE_U8 entry's
    single-FMA contract is written for quantized_tanh (the library answers QNN_EUNSUPPORTED), so the layer runs on the
    exact float32 path on bytes / 255, formed as the reference forms them (utils/load_data.py:40)."""
    if x.dtype == torch.uint8 and fn in _NEW_QUANT_FNS:
        return x.to(torch.float32) / F32(255)
    return x


def _join_store(act_bits, wstore):
    """Storage both operands of the next contraction are brought to."""
    astore = _abi.STORE_BIN if act_bits == 1 else _abi.store_for_bits(act_bits)
    if wstore is None:
        return None
    if astore == _abi.STORE_BIN and wstore == _abi.STORE_BIN:
        return _abi.STORE_BIN
    a = 0 if astore == _abi.STORE_BIN else astore
    w = 0 if wstore == _abi.STORE_BIN else wstore
    return max(a, w, _abi.STORE_I4)


def _weights_fit(op, store):
    """True if the weights of contraction `op` can be prepacked at packed activation store `store` (what _join_store
    arrives at; a tensor whose store the planner did not join with this op is contracted in float32 instead)."""
    ws = _wstore(op)
    if ws is None:
        return False
    if store == _abi.STORE_BIN:
        return ws == _abi.STORE_BIN
    if store == _abi.STORE_T2:
        return op["kind"] == "ternary"
    return ws == _abi.STORE_BIN or ws <= store


def _dilation(op):
    """dilation_rate of a conv op as a pair ((1, 1) where the spec says nothing: dense ops, ordinary windows); a dwconv op
    and a gconv op carry it as `dilation`."""
    d = op.get("dilation", (1, 1)) if op["op"] in ("dwconv", "gconv") else op.get("dilation_rate", (1, 1))
    return (int(d), int(d)) if np.isscalar(d) else (int(d[0]), int(d[1]))


def _matrix_pipe_1bit(op):
    """True if a 1-bit x 1-bit conv should take the int8 matrix pipe instead of XNOR+popcount.

    On MI355X the int8 MFMA kernel with register-resident operands (k_conv_mfma_areg: 3x3,
    Cin <= 128, one 64-filter slice) runs the CIFAR B0 layer in 34 us against 76 us for the
    XNOR kernel at 81 % of the popcount ceiling (profiles/r01), with bit-identical results:
    the +-1 codes are then stored as int4 between the layers (8 KB instead of 2 KB per image,
    far below any bandwidth limit).  VALU-only mode keeps the bit-packed path.
    """
    if _abi.conv_impl() == _abi.IMPL_VALU or op is None or op["op"] != "conv" or op["kind"] != "binary":
        return False
    kh, kw, cin, cout = op["kernel"].shape
    return kh == 3 and kw == 3 and cin in (64, 128) and cout == 64 and _dilation(op) == (1, 1)   # (that kernel has adjacent taps)


def _prepack(op, store, device, stride=1, same_pad=True):
    kernel = torch.as_tensor(np.ascontiguousarray(op["kernel"], dtype=F32)).to(device)
    bias = op.get("bias")
    bias = torch.as_tensor(np.ascontiguousarray(bias, dtype=F32)).to(device) if bias is not None else None
    if op["op"] == "dwconv":                 # Keras' depthwise kernel (kh, kw, C, depth_multiplier)
        M = int(op.get("depth_multiplier", kernel.shape[3]))
        if kernel.dim() != 4 or kernel.shape[3] != M:
            raise ValueError("dwconv: kernel %s does not match depth_multiplier %d" % (tuple(kernel.shape), M))
        return _abi.DepthwiseWeights(_wkind(op), int(op.get("nb", 1)), float(op.get("H", 1.0)), kernel, bias,
                                     stride, same_pad, store, dilation=_dilation(op))
    if op["op"] == "tconv":                  # Keras' Conv2DTranspose kernel (kh, kw, Cout, Cin)
        if kernel.dim() != 4:
            raise ValueError("tconv: kernel %s is not (kh, kw, Cout, Cin)" % (tuple(kernel.shape),))
        return _abi.TConvWeights(_wkind(op), int(op.get("nb", 1)), float(op.get("H", 1.0)), kernel, bias, stride, same_pad,
                                 store)
    if op["op"] == "gconv":                  # Keras' grouped kernel (kh, kw, Cin / groups, Cout)
        groups = int(op.get("groups", 1))
        if kernel.dim() != 4 or groups < 1 or kernel.shape[3] % groups != 0:
            raise ValueError("gconv: kernel %s is not (kh, kw, Cin / groups, Cout) for groups=%d" % (tuple(kernel.shape), groups))
        return _abi.GConvWeights(_wkind(op), int(op.get("nb", 1)), float(op.get("H", 1.0)), kernel, bias, groups, stride,
                                 same_pad, store, dilation=_dilation(op))
    return _abi.Weights(_wkind(op), int(op.get("nb", 1)), float(op.get("H", 1.0)), kernel, bias,
                        stride, same_pad, store, dilation=_dilation(op))


def _images(x, what):
    """The images of a forward as the C ABI takes them: uint8 (the typed QNN_STORE_U8 entry) or float32, NHWC on the GPU."""
    if isinstance(x, torch.Tensor) and x.dtype == torch.uint8:
        return _abi.require_cuda_u8(x, what)
    return _abi.require_cuda(x, what)


class _SpecGraph:
    """One reading of a net spec for the interpreters below: the name of every op's output, which op produces and which
    ops consume each tensor, the BN constants on the device, and the weights, prepacked when first asked for."""

    def __init__(self, spec, device):
        self.spec, self.device = spec, torch.device(device)
        self.names = [op.get("dst", "t%d" % i) for i, op in enumerate(spec)]
        self.prod = {n: i for i, n in enumerate(self.names)}
        # the tensors op i reads: add -> a, b; concat, merge -> their srcs; a named `src`; else the previous op's output; else
        # the images
        self.srcs = [[op["a"], op["b"]] if op["op"] == "add" else list(op["srcs"]) if op["op"] in ("concat", "merge") else
                     [op["src"] if "src" in op else self.names[i - 1] if i > 0 else "input"] for i, op in enumerate(spec)]
        self.cons = {}
        for i, ss in enumerate(self.srcs):
            for s in ss:
                self.cons.setdefault(s, []).append(i)
        self.bn = {i: tuple(torch.as_tensor(c).to(self.device) for c in bn_constants(op))
                   for i, op in enumerate(spec) if op["op"] == "bn"}
        self.packed = {}                     # (op index, store) -> _abi.Weights
        self.tails = {}                      # op index -> tail() of it
        self.tail_no = set()                 # tails (index of their last op) the library had no fused kernel for

    def _behind(self, name, kind):
        """Index of the op producing `name` if it is of `kind` and nothing else reads `name`."""
        i = self.prod.get(name)
        return i if i is not None and self.spec[i]["op"] == kind and len(self.cons.get(name, [])) == 1 else None

    def tail(self, i):
        """The classifier tail of models/resnet.py:134-140 that ends in op `i`, as (avgpool, flatten, dense, softmax or
        None) op indices, or None: `i` is a softmax, or a dense that is the spec's last op, behind dense <- flatten <-
        avgpool, every link read by the next one alone (nothing else needs the averages or the logits)."""
        if i not in self.tails:
            spec, t = self.spec, None
            sm = i if spec[i]["op"] == "softmax" else None
            de = self._behind(self.srcs[i][0], "dense") if sm is not None else \
                i if spec[i]["op"] == "dense" and i == len(spec) - 1 else None
            fl = self._behind(self.srcs[de][0], "flatten") if de is not None else None
            ap = self._behind(self.srcs[fl][0], "avgpool") if fl is not None else None
            if ap is not None and not _new_pool(spec[ap]):      # the fused tail is the size-only average
                t = (ap, fl, de, sm)
            self.tails[i] = t
        return self.tails[i]

    def tail_from(self, ap):
        """The tail() that starts at avgpool op `ap`, or None (for an interpreter that walks the spec front to back)."""
        def only(i, kind):
            c = self.cons.get(self.names[i], []) if i is not None else []
            return c[0] if len(c) == 1 and self.spec[c[0]]["op"] == kind else None
        de = only(only(ap, "flatten"), "dense")
        if de is None:
            return None
        sm = only(de, "softmax")
        t = self.tail(de if sm is None else sm)
        return t if t is not None and t[0] == ap else None

    def run_tail(self, t, src):
        """The tail `t` on the packed activation `src` in ONE launch (qnn_avgpool_dense_softmax_forward: bit-identical to
        avgpool_packed -> dense on the QNN_STORE_F32 handle -> softmax), or None where the library has no fused kernel
        (remembered: it is asked once) -- the caller then runs the ops one by one, as both interpreters did before."""
        ap, _, de, sm = t
        end = de if sm is None else sm
        if end in self.tail_no or src.store not in (_abi.STORE_BIN, _abi.STORE_I4, _abi.STORE_I8):
            return None
        try:
            return _abi.avgpool_dense_softmax(self.weights(de, _abi.STORE_F32), src.t, src.store, src.bits, *src.shape,
                                              self.spec[ap].get("size", 8), softmax=sm is not None)
        except _abi.QnnUnsupported:
            self.tail_no.add(end)
            return None

    def weights(self, i, store):
        if (i, store) not in self.packed:
            op = self.spec[i]
            self.packed[i, store] = _prepack(op, store, self.device, stride=tuple(op.get("strides", (1, 1)))[0],
                                             same_pad=op.get("padding", "same") == "same")
        return self.packed[i, store]


# ---- the stock Keras layers around the contractions, on float32 tensors.  Every interpreter below calls these, so their
# results cannot drift apart; oracle/qnn_oracle.py restates them independently.
# Pooling ops.  An op that carries only an integer `size` is the OLD FORM (a square window, strides equal to it,
# 'valid'): what every spec builder and reference checkpoint produces, run by the torch code below and fused as before.
# Anything else -- `size` as a pair, `strides`, `padding`, the two global ops -- is the NEW FORM: Keras' pooling with
# TensorFlow's padding (include/qnn_abi_pool.h), run by qnn_pool2d_forward on float32 here and on packed codes by the engines.
_POOLS = ("maxpool", "avgpool", "globalmaxpool", "globalavgpool")


def _new_pool(op):
    if op["op"] in ("globalmaxpool", "globalavgpool"):
        return True
    return op["op"] in ("maxpool", "avgpool") and ("strides" in op or "padding" in op or
                                                   not isinstance(op.get("size", 2), (int, np.integer)))


def _pool_run(x, store, bits, shape, op):
    """A new-form pooling op on an NHWC tensor `x` (float32, or packed words at (store, bits)) through
    qnn_pool2d_forward: (y, output shape); y is float32 for the averages, stored like x for the maxima.  The global ops
    are the whole image as the window and give (N, C)."""
    N, H, W, C = shape
    mode = _abi.POOL_MAX if op["op"] in ("maxpool", "globalmaxpool") else _abi.POOL_AVG
    if op["op"].startswith("global"):
        y, _, _ = _abi.pool2d(x, store, bits, N, H, W, C, mode, (H, W))
        return (y.reshape(N, C) if y.dtype == torch.float32 else y), (N, C)
    padding = str(op.get("padding", "valid")).lower()
    if padding not in ("valid", "same"):
        raise ValueError("%s: padding must be 'valid' or 'same', got %r" % (op["op"], op.get("padding")))
    y, Ho, Wo = _abi.pool2d(x, store, bits, N, H, W, C, mode, op.get("size", 2 if mode == _abi.POOL_MAX else 8),
                            op.get("strides"), padding == "same")
    return y, (N, Ho, Wo, C)


def _pool_f32(t, op):
    return _pool_run(t.contiguous(), _abi.STORE_F32, 0, t.shape, op)[0]


def _maxpool(t, op):
    if _new_pool(op):
        return _pool_f32(t, op)
    s = op.get("size", 2)
    N, H, W, C = t.shape
    return t[:, :H // s * s, :W // s * s, :].reshape(N, H // s, s, W // s, s, C).amax(dim=(2, 4))


def _avgpool(t, op):
    if _new_pool(op):
        return _pool_f32(t, op)
    s = op.get("size", 8)
    N, H, W, C = t.shape
    win = t[:, :H // s * s, :W // s * s, :].reshape(N, H // s, s, W // s, s, C)
    # window sums of grid values are exact in float64; one division in float32
    return win.double().sum(dim=(2, 4)).float() / F32(s * s)


# Spatial ops (include/qnn_abi_spatial.h): every output pixel is a copy of one input pixel or zero.  A zeropad op whose
# `pad` is one integer is the OLD FORM (what every spec builder and reference checkpoint produces, run by the torch code
# below on float32); `pad` as ((top, bottom), (left, right)), `crop` and `upsample` are the NEW FORM, run by
# qnn_spatial2d_forward on float32 here and on packed codes by GraphModel.
_SPATIAL = ("zeropad", "crop", "upsample")


def _new_spatial(op):
    if op["op"] == "zeropad":
        return not isinstance(op["pad"], (int, np.integer))
    return op["op"] in ("crop", "upsample")


def _spatial_steps(op):
    """The steps of qnn_spatial2d_t a new-form spatial op sets."""
    if op["op"] == "upsample":
        return {"up": _abi._pair(op["size"], "size")}
    key = "pad" if op["op"] == "zeropad" else "crop"
    v = op[key]
    if not (isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(side, (tuple, list)) and len(side) == 2 for side in v)):
        raise ValueError("%s: `%s` is ((top, bottom), (left, right))%s, got %r"
                         % (op["op"], key, " or one integer" if key == "pad" else "", v))
    t, b, l, r = _abi.pairs2d(v, key)
    return {key: ((t, b), (l, r))}


def _spatial_run(x, store, bits, shape, op, log=None):
    """A new-form spatial op on an NHWC tensor `x` (float32, or packed words at (store, bits)): (y, output shape)."""
    N, H, W, C = shape
    y, Ho, Wo = _abi.spatial2d(x, store, bits, N, H, W, C, **_spatial_steps(op))
    if log is not None:
        log.append(_abi.last_kernel())
    return y, (N, Ho, Wo, C)


def _spatial_f32(t, op):
    return _spatial_run(t.contiguous(), _abi.STORE_F32, 0, t.shape, op)[0]


def _zeropad(t, op):
    if _new_spatial(op):
        return _spatial_f32(t, op)
    p = op["pad"]
    return torch.nn.functional.pad(t, (0, 0, p, p, p, p))


def _refuse_spatial(spec, who):
    """The fused engines plan their launches over conv -> BN -> clip chains and size-only pools; GraphModel runs a spec
    that resizes a map between them."""
    for op in spec:
        if op["op"] in _SPATIAL and _new_spatial(op):
            raise _abi.NotFusable("%s: op %r (%s) is not expressed by this engine; use GraphModel"
                                  % (who, op["op"], "pair-form zero padding" if op["op"] == "zeropad" else
                                     "cropping" if op["op"] == "crop" else "nearest-neighbour up-sampling"))


def _flatten(t, op):
    return t.reshape(t.shape[0], -1)


def _scale(t, op):
    return t * F32(op["value"])


def _add(a, b):
    return a + b


def _concat_run(tensors, channels, store, bits, pixels, log=None):
    """qnn_concat_forward over any number of inputs: more than it takes in one call are joined front to back, the
    result so far as the first input of the next call."""
    tensors, channels = list(tensors), list(channels)
    while True:
        k = _abi.CONCAT_MAX
        y = _abi.concat(tensors[:k], channels[:k], store, bits, pixels)
        if log is not None:
            log.append(_abi.last_kernel())
        if len(tensors) <= k:
            return y
        tensors, channels = [y] + tensors[k:], [sum(channels[:k])] + channels[k:]


def _concat_shapes(shapes, what="concat"):
    """The shape of the channel concatenation of tensors shaped `shapes` (ValueError unless they differ in the last axis only)."""
    shapes = [tuple(int(d) for d in s) for s in shapes]
    if len({s[:-1] for s in shapes}) != 1:
        raise ValueError("%s: the inputs must have matching shapes except for the channel axis, got %s" % (what, shapes))
    return shapes[0][:-1] + (sum(s[-1] for s in shapes),)


def _concat_f32(tensors, log=None):
    """Concatenate(axis=-1) of float32 tensors (concat_f32)."""
    shape = _concat_shapes([t.shape for t in tensors])
    y = _concat_run([t.contiguous() for t in tensors], [t.shape[-1] for t in tensors], _abi.STORE_F32, 0,
                    math.prod(shape[:-1]), log)
    return y.reshape(shape)


def _merge_shape(shapes, op):
    """The one shape of the tensors a merge op reads (QnnError naming the shapes unless they are identical: Keras would
    broadcast) after the checks on their number."""
    fn = op.get("fn")
    if fn not in _abi.MERGE_OPS:
        raise ValueError("merge: fn=%r (one of %s)" % (fn, ", ".join(_abi.MERGE_OPS)))
    shapes = [tuple(int(d) for d in s) for s in shapes]
    if not 2 <= len(shapes) <= _abi.MERGE_MAX or (fn == "sub" and len(shapes) != 2):
        raise ValueError("merge %r: %d sources (2 .. %d; 'sub': exactly 2)" % (fn, len(shapes), _abi.MERGE_MAX))
    if len(set(shapes)) != 1:
        raise _abi.QnnError("merge %r: sources of shapes %s; only identical shapes are supported (no broadcasting)" % (fn, shapes))
    return shapes[0]


def _merge_f32(tensors, op, log=None):
    """A merge op on float32 tensors (merge_f32): Keras' left-to-right chain."""
    shape = _merge_shape([t.shape for t in tensors], op)
    y = _abi.merge([t.contiguous() for t in tensors], op["fn"], _abi.STORE_F32, 0, math.prod(shape[:-1]), shape[-1])[0]
    if log is not None:
        log.append(_abi.last_kernel())
    return y.reshape(shape)


# Packed forms that GraphModel sends through float32 instead (unpack -> merge_f32): the ones measured slower than that
# route beyond its own spread (profiles/merge/README.md).  (fn, store) pairs.
_MERGE_F32_ROUTE = frozenset()


def _refuse_merge(spec, who):
    """The fused engines plan one tensor per op (an add: two, as the ResNet shortcut); GraphModel (and LayerModel) run a
    spec whose branches meet in a Keras merge layer."""
    if any(op["op"] == "merge" for op in spec):
        raise _abi.NotFusable("%s: op 'merge' (element-wise merge of branches) is not expressed by this engine; use GraphModel" % who)


def _refuse_dwconv(spec, who):
    """The fused engines plan full convolutions only: a spec that holds a depthwise convolution runs on GraphModel."""
    if any(op["op"] == "dwconv" for op in spec):
        raise _abi.NotFusable("%s: op 'dwconv' (depthwise convolution) is not expressed by this engine; use GraphModel" % who)


def _refuse_gconv(spec, who):
    """The packed engines express a chain of full convolutions; a grouped convolution runs in GraphModel (and LayerModel)."""
    if any(op["op"] == "gconv" for op in spec):
        raise _abi.NotFusable("%s: op 'gconv' (grouped convolution) is not expressed by this engine; use GraphModel" % who)


def _refuse_tconv(spec, who):
    """The fused engines plan forward convolutions only: a spec that holds a transposed convolution runs on GraphModel."""
    if any(op["op"] == "tconv" for op in spec):
        raise _abi.NotFusable("%s: op 'tconv' (transposed convolution) is not expressed by this engine; use GraphModel" % who)


def _refuse_concat(spec, who):
    """The fused engines and the layer-by-layer one read one tensor per op (an add: two); GraphModel runs a spec whose
    branches meet by stacking channels."""
    if any(op["op"] == "concat" for op in spec):
        raise _abi.NotFusable("%s: op 'concat' (channel concatenation) is not expressed by this engine; use GraphModel" % who)


def _bn_apply(t, inv, shift):
    return t * inv + shift                   # two roundings, as tf.nn.batch_normalization


def _act(t, op):
    """An activation op: the clips of layers/*_ops.py (ternary_tanh thresholds at the mean of the whole batch tensor,
    ternary_ops.py:23; quantized_maxrelu / quantized_leakymaxrelu scale by its maximum, quantized_ops.py:134: each batch
    a model is called on is quantised with its own maximum, as the reference's predict(batch_size) does) and LeakyReLU."""
    fn = op["fn"]
    if fn == "binary_tanh":
        return binary_ops.binary_tanh(t)
    if fn == "quantized_tanh":
        return quantized_ops.quantized_tanh(t, op["nb"])
    if fn == "quantized_relu":
        return quantized_ops.quantized_relu(t, op["nb"])
    if fn == "quantized_leakyrelu":
        return quantized_ops.quantized_leakyrelu(t, op["nb"], op.get("alpha", quantized_ops.LEAKY_ALPHA))
    if fn == "quantized_maxrelu":
        return quantized_ops.quantized_maxrelu(t, op["nb"])
    if fn == "quantized_leakymaxrelu":
        return quantized_ops.quantized_leakymaxrelu(t, op["nb"], op.get("alpha", quantized_ops.LEAKY_ALPHA))
    if fn == "ternary_tanh":
        return ternary_ops.ternary_tanh(t)
    if fn == "leaky_relu":
        return torch.where(t >= 0, t, t * F32(op.get("alpha", 0.3)))
    raise ValueError(fn)


_GLUE = {"maxpool": _maxpool, "avgpool": _avgpool, "globalmaxpool": _pool_f32, "globalavgpool": _pool_f32, "zeropad": _zeropad, "crop": _spatial_f32, "upsample": _spatial_f32, "flatten": _flatten, "scale": _scale, "act": _act,
         "softmax": lambda t, op: _abi.softmax(t)}


class _DomainFlag:
    """The "auto" first layer of the two fused engines: float32 images run on the byte kernel, which raises a domain-flag
    word (qnn_epilogue_t.domain_flag) when a value is not an image byte / 255; a flagged batch is recomputed on the exact
    kernel.  An engine passes _own_flag() to its first layer where _auto_now(images) holds, gives `_forward(x)` (one
    forward as `first_layer` and `_exact_now` say), `_check_restricted()` and the text `_UNRECOMPUTED`."""

    _flag = None                             # the word the first layer writes: the model's own unless flag_word() says otherwise
    _exact_now = False                       # the batch being recomputed takes the exact kernel

    def _auto_now(self, x):
        return self.first_layer == "auto" and not self._exact_now and x.dtype == torch.float32

    def _own_flag(self):
        if self._flag is None:
            self._flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._flag

    @contextlib.contextmanager
    def flag_word(self, word):
        """Inside the block the first layer writes `word` (an int32 device tensor) instead of the model's own word, which
        keeps what it holds: a raise an earlier replay left there unread, or none where the block's batch raises one."""
        own, self._flag = self._flag, word
        try:
            yield word
        finally:
            self._flag = own

    def take_flag(self):
        """Synchronise, return True and clear if this model's own flag word is raised (an eager forward, a captured graph
        or a bench replay met a batch that is not image bytes / 255)."""
        if self._flag is None:
            return False
        raised = int(self._flag.item()) != 0
        if raised:
            self._flag.zero_()
        return raised

    def forward(self, x):
        """x: float32 or uint8 NHWC CUDA tensor -> the network's output, float32."""
        y = self._forward(x)
        if self._auto_now(x) and not torch.cuda.is_current_stream_capturing() and self.take_flag():
            y = self.forward_exact(x)        # the batch was not image bytes / 255
        return y

    def forward_exact(self, x, **kw):
        """The forward with the exact float32 first layer, whatever `first_layer` says (what "auto" falls back to)."""
        self._exact_now = True
        try:
            return self._forward(x, **kw)
        finally:
            self._exact_now = False

    def check_domain(self):
        """Synchronise the current stream and raise QnnError if a restricted-domain first layer ("fixed", "image") met
        an input outside its domain since the last check (qnn_weights_check).  "auto": raises only for replays nobody
        recomputed (hipGraph replays outside engine.Pipelined.forward).  A no-op for the exact and uint8 entries."""
        if self.first_layer != "auto":
            self._check_restricted()
        elif self.take_flag():
            raise _abi.QnnError(self._UNRECOMPUTED)

    __call__ = forward
    predict = forward


# ---------------------------------------------------------------------------
class FusedModel(_DomainFlag):
    """Packed, fully fused pipeline for sequential specs (models/vgg.py topology).

    forward(x) takes the images either as uint8 NHWC, the dataset's own bytes (value = code / 255,
    utils/load_data.py:40: the typed QNN_STORE_U8 entry of the C ABI, an exact integer first layer), or as float32
    NHWC, where `first_layer` picks the kernel:
      "auto"   any float32 values (default): a batch is first run on the byte kernel of "image" with a domain-flag word
               of its own (qnn_epilogue_t.domain_flag); a batch that turns out NOT to be image bytes / 255 is recomputed,
               in-process, on the exact kernel.  Like the reference's call() (quantized_layers.py:164-194) it accepts
               every float tensor; dataset images (utils/load_data.py:40) take the fast kernel.
      "exact"  any float32 values: the float32 FMA chain the oracle evaluates;
      "image"  float32 values that are image bytes / 255: recognised as bytes, computed like the uint8 entry;
      "fixed"  float32 values in [0, 1]: fixed point at 2^-23.
    "image" and "fixed" have restricted domains; a value outside raises the layer's domain flag, which surfaces as
    QnnError from check_domain() (or from the next forward once the host has seen it) -- never silently."""

    # how float32 images are declared to the C ABI: a typed entry per call, no process-wide switch is touched
    FIRST_LAYER_STORE = {"exact": _abi.STORE_F32, "image": _abi.STORE_F32_IMAGE, "fixed": _abi.STORE_F32_UNIT,
                         "auto": _abi.STORE_F32_IMAGE}
    _UNRECOMPUTED = ("FusedModel: a replayed batch was not image bytes / 255 and has not been recomputed on "
                     "the exact first layer (run it through forward() / engine.Pipelined.forward())")

    def __init__(self, spec, device="cuda", first_layer="auto", trick=None):
        """trick: None = the reference's lr-multiplier identity trick is the identity ("exact" mode, the default), or
        "nep50" / "legacy" = its OUTPUT side (binary_layers.py:175-176) is replayed in float32 behind every low-bit
        conv with the constants the reference forms under that numpy promotion rule (qnn_abi.h, trick_c / trick_s):
        reproduces the reference's rounding noise on 8-bit activation grids at the price of the VALU kernel family."""
        if first_layer not in self.FIRST_LAYER_STORE:
            raise ValueError("first_layer must be 'auto', 'exact', 'image' or 'fixed', got %r" % (first_layer,))
        if trick not in (None, "nep50", "legacy"):
            raise ValueError("trick must be None, 'nep50' or 'legacy', got %r" % (trick,))
        if first_layer == "auto" and trick is not None:
            first_layer = "exact"            # the faithful output-side trick lives in the VALU kernel family only
        self.first_layer = first_layer
        self.fold = True                     # folded epilogues where the library proves one (today: the image entry's first layer)
        self.device = torch.device(device)
        self.fuse_head = True                # conv group + Flatten + Dense in one launch where the library has the kernel
        self._head_no = {}                   # (H, W) of inputs the library has no fused head kernel for
        self.steps = []
        self._keep = []
        _refuse_concat(spec, "FusedModel")
        _refuse_merge(spec, "FusedModel")
        _refuse_dwconv(spec, "FusedModel")
        _refuse_tconv(spec, "FusedModel")
        _refuse_gconv(spec, "FusedModel")
        _refuse_spatial(spec, "FusedModel")
        _refuse_max_acts(spec, "FusedModel")
        groups = self._group(spec)
        if groups is None:
            raise _abi.NotFusable("FusedModel: spec is not a fusable chain; use GraphModel")
        x_store, x_bits = _abi.STORE_F32, 0
        for gi, g in enumerate(groups):
            op = g["op"]
            nxt = groups[gi + 1]["op"] if gi + 1 < len(groups) else None
            store_in = x_store
            if store_in != _abi.STORE_F32 and _wstore(op) is None:
                raise _abi.NotFusable("FusedModel: float layer after a packed tensor")
            w = _prepack(op, store_in, self.device, stride=g["stride"], same_pad=g["same"])
            inv = shift = None
            if g["bn"] is not None:
                i, s = bn_constants(g["bn"])
                inv = torch.as_tensor(i).to(self.device)
                shift = torch.as_tensor(s).to(self.device)
                self._keep += [inv, shift]
            ac = _act_code(g["act"])
            if g["act"] is not None and ac is None:
                raise _abi.NotFusable("FusedModel: activation %r cannot be fused" % g["act"]["fn"])
            if ac is None:
                fn, bits, out_store = _abi.FN_NONE, 0, _abi.STORE_F32
                if nxt is not None:
                    raise _abi.NotFusable("FusedModel: layer without a low-bit activation mid-chain")
            else:
                fn, bits = ac
                out_store = _join_store(bits, _wstore(nxt)) if nxt is not None else _abi.STORE_F32
                if out_store is None:
                    raise _abi.NotFusable("FusedModel: float layer after a low-bit activation")
                if out_store == _abi.STORE_BIN and _matrix_pipe_1bit(nxt):
                    out_store = _abi.STORE_I4
                if g["kind"] == "conv" and nxt is not None and nxt["op"] == "dense":
                    # Flatten of a packed tensor is a no-op only when every pixel's channels fill whole
                    # words: the conv pads each pixel to a word boundary, the dense weights are packed as
                    # one contiguous K = H*W*C vector.  Widen the storage until the channels divide.
                    cout = op["kernel"].shape[3]
                    kh_, kw_, cin_, _ = op["kernel"].shape
                    if out_store == _abi.STORE_BIN and (kh_, kw_, cout) == (3, 3, 64) and cin_ in (64, 128) and \
                            g["pool"] == 2 and g["stride"] == 1 and g["same"] and x_store == _abi.STORE_I4 and \
                            _dilation(op) == (1, 1) and \
                            nxt["kernel"].shape[0] == 1024 and nxt["kernel"].shape[1] <= 16 and \
                            _abi.conv_impl() != _abi.IMPL_VALU:
                        # +-1 codes as int4 in front of the classifier: lets the last conv group and the dense layer
                        # run as ONE launch (qnn_conv2d_dense_forward); 8 KB instead of 2 KB per image, never stored
                        out_store = _abi.STORE_I4
                    while cout % _abi.per_word(out_store) != 0 and out_store < _abi.STORE_I8:
                        out_store = {_abi.STORE_BIN: _abi.STORE_I4, _abi.STORE_I4: _abi.STORE_I8}[out_store]
                    if cout % _abi.per_word(out_store) != 0:
                        raise _abi.NotFusable("FusedModel: %d channels in front of Flatten do not fill whole "
                                              "packed words" % cout)
            tk = None
            if trick is not None and g["kind"] == "conv" and op["kind"] in ("binary", "quantized"):
                kh_, kw_, ci_, co_ = op["kernel"].shape
                klm = op.get("klm")
                if klm is None:
                    klm = np.float32(1.0 / np.sqrt(1.5 / (int(ci_ * kh_ * kw_) + int(co_ * kh_ * kw_))))
                tk = _abi.faithful_trick(klm, trick)
            self.steps.append(dict(kind=g["kind"], w=w, x_store=x_store, x_bits=x_bits, inv=inv,
                                   shift=shift, fn=fn, act_bits=bits if fn in _abi.QUANT_FNS else 0,
                                   pool=g["pool"], out_store=out_store, softmax=g.get("softmax", False), trick=tk))
            x_store, x_bits = out_store, bits

    @staticmethod
    def _group(spec):
        """[conv|dense] [bn] [act] [maxpool] ... -> list of groups, or None."""
        groups, i, n = [], 0, len(spec)
        seen_dense = False
        while i < n:
            op = spec[i]
            if "src" in op and i > 0:
                return None
            if op["op"] == "flatten":
                i += 1
                continue
            if op["op"] not in ("conv", "dense"):
                return None
            g = dict(op=op, kind=op["op"], bn=None, act=None, pool=1, stride=1, same=True)
            if op["op"] == "conv":
                if seen_dense:
                    return None
                st = tuple(op.get("strides", (1, 1)))
                if st[0] != st[1]:
                    return None
                g["stride"] = st[0]
                g["same"] = op.get("padding", "same") == "same"
            else:
                seen_dense = True
            i += 1
            if i < n and spec[i]["op"] == "bn":
                g["bn"] = spec[i]; i += 1
            if i < n and spec[i]["op"] == "act":
                g["act"] = spec[i]; i += 1
            if i < n and spec[i]["op"] == "maxpool":
                if _new_pool(spec[i]) or spec[i].get("size", 2) != 2 or g["kind"] != "conv":
                    return None                  # (a new-form pool is never the 2x2 / 2 epilogue pool, whatever its size)
                g["pool"] = 2; i += 1
            if i < n and spec[i]["op"] == "softmax":
                g["softmax"] = True; i += 1
            groups.append(g)
        return groups

    def _head_candidate(self):
        """True if the last two steps are a pooled conv group with int4 output and the dense head behind it (the shape
        qnn_conv2d_dense_forward fuses; the library decides about the exact geometry at launch)."""
        if not self.fuse_head or len(self.steps) < 2:
            return False
        c, d = self.steps[-2], self.steps[-1]
        return (c["kind"] == "conv" and d["kind"] == "dense" and c["pool"] == 2 and c["out_store"] == _abi.STORE_I4
                and c["x_store"] == _abi.STORE_I4 and d["x_store"] == _abi.STORE_I4 and d["out_store"] == _abi.STORE_F32
                and d["fn"] == _abi.FN_NONE and not d["softmax"] and not c["softmax"] and c["trick"] is None
                and c["fn"] not in _NEW_QUANT_FNS
                and c["w"].dilation == (1, 1)
                and _abi.conv_impl() != _abi.IMPL_VALU)

    def run_head(self, cur, N, H, W, out=None):
        """The last conv group and the classifier in one launch (qnn_conv2d_dense_forward); None if the library has no
        fused kernel for this geometry -- the caller then runs the two steps one after the other."""
        if not self._head_candidate() or self._head_no.get((H, W)):
            return None
        c, d = self.steps[-2], self.steps[-1]
        y = _abi.conv2d_dense(c["w"], d["w"], cur, c["x_store"], c["x_bits"], N, H, W, c["inv"], c["shift"], c["fn"],
                              c["act_bits"], d["inv"], d["shift"], out=out,
                              fold=self._first_fold(len(self.steps) - 2, c["x_store"]))
        if y is None:
            self._head_no[(H, W)] = True     # no fused kernel for this geometry: do not ask again
        return y

    def run_step(self, si, cur, N, H, W, out=None):
        """Launch step `si` on `cur` (the images for si = 0: float32 or uint8; else the previous step's output).
        Returns (output, H, W).  forward() is this in a loop; bench.py times the steps one by one through it."""
        st = self.steps[si]
        if st["kind"] != "conv":
            return _abi.dense(st["w"], cur, st["x_store"], st["x_bits"], N, st["inv"], st["shift"],
                              st["fn"], st["act_bits"], st["out_store"], out=out), H, W
        if si == 0:
            cur = _float_images(cur, st["fn"])
        u8 = si == 0 and cur.dtype == torch.uint8
        if u8 and st["trick"] is not None:
            #  never drop the faithful trick silently: the uint8 entry has no output-side trick
            raise _abi.QnnError("FusedModel: trick=%r cannot be combined with uint8 images (the QNN_STORE_U8 entry has no "
                                "output-side trick); pass float32 images" % (st["trick"],))
        x_store = _abi.STORE_U8 if u8 else self._x_store(si)
        flag = self._own_flag() if (si == 0 and self._auto_now(cur)) else None
        return _abi.conv2d(st["w"], cur, x_store, st["x_bits"], N, H, W, st["inv"],
                           st["shift"], st["fn"], st["act_bits"], st["pool"], st["out_store"], out=out,
                           trick=st["trick"], domain_flag=flag, fold=self._first_fold(si, x_store))

    def _first_fold(self, si, x_store):
        """The folded epilogue of step `si` for a call with input store `x_store` (qnn_fold_prepare: proven equal to the
        float32 chain / the image entry's specification on the layer's whole accumulator domain), prepared once per
        (step, form); None where nothing is folded (other stores or bit widths, float32 output, the faithful trick).
          step 0 on image bytes (uint8, "image" / "auto")  -> the image entry's form (mode 3);
          int4 -> int4 layers with quantized_tanh(4)          -> the matrix-pipe forms (modes 1 / 2)."""
        st = self.steps[si]
        if not self.fold or st["kind"] != "conv" or st["fn"] != _abi.FN_QUANTIZED_TANH or st["act_bits"] != 4 or \
                st["out_store"] != _abi.STORE_I4 or st["trick"] is not None or st["w"].dilation != (1, 1):
            return None
        if si == 0 and x_store in (_abi.STORE_U8, _abi.STORE_F32_IMAGE):
            key, args = "fold_img", (_abi.STORE_U8, 0)
        elif x_store == _abi.STORE_I4:
            key, args = "fold_i4", (_abi.STORE_I4, st["x_bits"])
        else:
            return None
        if key not in st:
            if torch.cuda.is_current_stream_capturing():
                return None                  # preparing synchronises: never inside a capture (the chain gives the same bits)
            st[key] = _abi.Fold.try_prepare(st["w"], args[0], args[1], st["inv"], st["shift"], st["fn"], 4, st["out_store"])
        return st[key]

    def _x_store(self, si):
        """Input store of step si for float32 / packed inputs (the first step carries the declared image domain)."""
        st = self.steps[si]
        if si == 0 and st["x_store"] == _abi.STORE_F32:
            return _abi.STORE_F32 if self._exact_now else self.FIRST_LAYER_STORE[self.first_layer]
        return st["x_store"]

    def bind(self, example):
        """A launch plan for batches shaped like `example`: every step bound to static intermediate tensors
        (_abi.BoundStep), so a forward is len(steps) foreign calls on a given stream with the caller's input and output
        pointers -- no allocation, no Python per layer, nothing copied.  Returns (plan, logits shape); plan(stream,
        x_ptr, y_ptr) enqueues one forward.  None if a step needs a torch op (softmax)."""
        if any(st["softmax"] for st in self.steps):
            return None
        if example.dtype == torch.uint8 and self.steps[0]["fn"] in _NEW_QUANT_FNS:
            return None                      # the bytes are divided by 255 in a torch op first (_float_images)
        N, H, W, _ = example.shape
        u8 = example.dtype == torch.uint8
        cur, bound = example, []
        nsteps = len(self.steps)
        # The binding pass runs the forward once on `example` only to create and bind the intermediates; its first
        # layer writes a scratch domain-flag word ("auto").  `example` need not be image bytes / 255 (engine.Pipelined
        # binds on the first batch of a new shape) and nothing reads this pass's flag: a raise left in the model's own
        # word would send the next eager forward of an image batch to the exact kernel and make check_domain() raise.
        # A scratch word rather than clearing the model's word afterwards: that would also erase a raise an earlier
        # replay left there unread.
        with self.flag_word(torch.zeros(1, dtype=torch.int32, device=self.device)):
            for si, st in enumerate(self.steps):
                if si == nsteps - 2 and si >= 1:
                    y = self.run_head(cur, N, H, W)
                    if y is not None:            # conv group + classifier in one launch: the plan ends here
                        c, d = self.steps[-2], self.steps[-1]
                        bound.append(_abi.BoundHead(c["w"], d["w"], c["x_store"], c["x_bits"], N, H, W, c["inv"], c["shift"],
                                                    c["fn"], c["act_bits"], d["inv"], d["shift"], cur,
                                                    fold=self._first_fold(len(self.steps) - 2, c["x_store"])))
                        cur = y
                        break
                out, H1, W1 = self.run_step(si, cur, N, H, W)
                x_store = _abi.STORE_U8 if (u8 and si == 0) else self._x_store(si)
                bound.append(_abi.BoundStep(st["kind"], st["w"], x_store, st["x_bits"], N, H, W, st["inv"], st["shift"],
                                            st["fn"], st["act_bits"], st["pool"], st["out_store"],
                                            None if si == 0 else cur, None if si == len(self.steps) - 1 else out,
                                            trick=None if (u8 and si == 0) else st["trick"],
                                            fold=self._first_fold(si, x_store) if st["kind"] == "conv" else None))
                cur, H, W = out, H1, W1
        last = len(bound) - 1
        own = self._own_flag().data_ptr() if self._auto_now(example) else None

        def plan(stream, x_ptr, y_ptr, flag_ptr=None):
            """flag_ptr ("auto" first layer): device address of THIS batch's domain-flag word (default: the model's)."""
            for i, b in enumerate(bound):
                if i == 0 and own is not None:
                    b(stream, x_ptr, y_ptr if i == last else None, flag_ptr or own)
                else:
                    b(stream, x_ptr if i == 0 else None, y_ptr if i == last else None)
        return plan, tuple(cur.shape), cur.dtype

    def forward_from(self, s0, cur, N, H, W, out=None):
        """Steps s0.. on `cur` (the images for s0 = 0, else the output of step s0 - 1 at H x W).  `out`: a tensor the
        last step writes its result into (only where no torch op follows it)."""
        log = getattr(self, "kernel_log", None)      # tests: set to a list to record the kernel of every layer
        last = len(self.steps) - 1
        if out is not None and self.steps[last]["softmax"]:
            raise _abi.QnnError("forward_from: `out` needs a network that ends in a library kernel")
        for si in range(s0, len(self.steps)):
            if si == last - 1 and last >= 1:
                y = self.run_head(cur, N, H, W, out=out)
                if y is not None:
                    if log is not None:
                        log += [_abi.last_kernel(), "(fused into the conv)"]
                    return y
            cur, H, W = self.run_step(si, cur, N, H, W, out=out if si == last else None)
            if log is not None:
                log.append(_abi.last_kernel())
            if self.steps[si]["softmax"]:
                cur = _abi.softmax(cur)
        return cur

    def _forward(self, x, out=None):
        what = "FusedModel.forward_exact" if self._exact_now else "FusedModel.forward"
        x = _abi.require_cuda(x, what) if self._exact_now else _images(x, what)
        if x.dtype == torch.uint8 and (self.steps[0]["kind"] != "conv" or self.steps[0]["w"].wkind == _abi.W_FLOAT):
            raise _abi.QnnError("FusedModel.forward: uint8 images need a low-bit convolution as the first layer")
        N, H, W, _ = x.shape
        return self.forward_from(0, x, N, H, W, out=out)

    def _check_restricted(self):
        self.steps[0]["w"].check()


# ---------------------------------------------------------------------------
class _Virtual:
    """An activation clip that has not been materialised: (pre-activation, fn, nb) of activation `op`."""

    def __init__(self, pre, fn, nb, op):
        self.pre, self.fn, self.nb, self.op = pre, fn, nb, op
        self._mat = None

    def materialize(self):
        if self._mat is None:                       # FN_GRID: already clipped (ternary_tanh), the values ARE the grid
            self._mat = self.pre if self.fn == _abi.FN_GRID else _act(self.pre, self.op)
        return self._mat


class _Scaled:
    """A batch-scaled activation (quantized_maxrelu / quantized_leakymaxrelu at nb <= 8) carried as packed codes plus the
    device-resident scale (include/qnn_abi_scaled.h): `packs` store -> int32 words, `ws` the 16-byte workspace whose word
    every scaled consumer reads (this object keeps it alive, and nothing writes it again: each activation has its own),
    `f32` the float32 tensor of the same pass for the consumers that need one (None: formed on demand from `pre`)."""

    def __init__(self, pre, fn, nb, ws, packs, f32, shape):
        self.pre, self.fn, self.nb, self.ws, self.packs, self.f32, self.shape = pre, fn, nb, ws, packs, f32, tuple(shape)
        self.parent = None                   # flat(): the NHWC tensor this one is a view of

    def materialize(self):
        if self.f32 is None and self.parent is not None:     # one float32 tensor serves both shapes
            self.f32 = self.parent.materialize().reshape(self.shape)
        if self.f32 is None:
            self.f32 = torch.empty_like(self.pre)
            _abi.check(_abi.load().qnn_maxact_apply_f32(_abi.ptr(self.pre), _abi.ptr(self.f32), self.pre.numel(), self.fn,
                                                        self.nb, _abi.ptr(self.ws), _abi.stream_ptr()), "qnn_maxact_apply_f32")
        return self.f32

    def flat(self):
        """Behind a Flatten: the same words read as (N, H * W * words) -- whole words per pixel only (_scaled_flat_ok)."""
        n = self.shape[0]
        v = _Scaled(self.pre.reshape(n, -1), self.fn, self.nb, self.ws, {s: p.reshape(n, -1) for s, p in self.packs.items()},
                    None if self.f32 is None else self.f32.reshape(n, -1), (n, math.prod(self.shape[1:])))
        v.parent = self
        return v


class GraphModel:
    """General spec interpreter on the GPU (see module docstring)."""

    # Default of `scaled_codes`: False.  Neither benchmark network has a consumer that takes the scaled route (ResNet-20's
    # convolutions stay on k_conv_f32act, _scaled_route_pays; the VGG's activations feed max-pools), so the measurement the
    # default was to be decided by shows no gain.  profiles/scaled/README.md.
    def __init__(self, spec, device="cuda", scaled_codes=False):
        self.device = torch.device(device)
        self.spec = spec
        self.graph = _SpecGraph(spec, device)
        self.fuse_tail = True                # avg-pool + Flatten + Dense [+ softmax] in one launch (_SpecGraph.run_tail)
        self.kernel_log = None               # tests: set to a list to record the kernel of every new-form pooling op, of every
                                             # concat and new-form spatial op ("unpack" in front of one that left the codes), and
                                             # of the pack and the consumers of every activation carried as scaled codes
        self.scaled_codes = bool(scaled_codes)
        self._scaled_memo = {}               # (op index, nb, input shape) -> _scaled_store: static per spec and shape

    # ---- batch-scaled activations as packed codes plus a device-resident scale (include/qnn_abi_scaled.h) ----
    def _scaled_store(self, c, nb, shape):
        """Packed store at which contraction op `c` may consume the nb-bit scaled codes of a tensor of `shape`, or None:
        low-bit weights, the input rank the op takes, and the exactness rule (scaled_route_exact)."""
        key = (c, nb, tuple(shape))
        if key not in self._scaled_memo:
            self._scaled_memo[key] = self._scaled_store_of(c, nb, shape)
        return self._scaled_memo[key]

    def _scaled_store_of(self, c, nb, shape):
        op = self.spec[c]
        wstore = _wstore(op) if op["op"] in ("conv", "dense") else None
        if wstore is None or len(shape) != (4 if op["op"] == "conv" else 2):
            return None
        k = op["kernel"].shape
        if int(k[-2]) != int(shape[-1]) or not scaled_route_exact(math.prod(k[:-1]), nb, op["nb"] if op["kind"] == "quantized" else 1):
            return None
        store = _join_store(nb, wstore)
        if not _weights_fit(op, store) or not _scaled_route_pays(op, store):
            return None
        return store

    def _scaled_plan(self, name, nb, shape):
        """(stores to pack at, True if some consumer needs the float32 tensor) for activation tensor `name`.  A Flatten
        read only by qualifying dense layers is looked through when the channels fill whole words."""
        g, stores, f32 = self.graph, set(), name == self.graph.names[-1]
        for c in g.cons.get(name, []):
            s = self._scaled_store(c, nb, shape)
            ss = {s} if s is not None else self._scaled_flat_ok(c, nb, shape)
            if ss is None:
                f32 = True
            else:
                stores |= ss
        return sorted(stores), f32

    def _scaled_flat_ok(self, c, nb, shape):
        """The stores behind Flatten op `c` if nothing but qualifying dense layers reads it and the channels fill whole
        words (the packed words of an NHWC tensor are then those of its flattened form), else None."""
        g = self.graph
        if self.spec[c]["op"] != "flatten" or len(shape) != 4 or g.names[c] == g.names[-1]:
            return None
        behind = g.cons.get(g.names[c], [])
        ss = {self._scaled_store(d, nb, (shape[0], math.prod(shape[1:]))) for d in behind}
        if not behind or None in ss or any(shape[-1] % _abi.per_word(t) for t in ss):
            return None
        return ss

    def _scaled_act(self, op, pre, name):
        """Activation op `op` on `pre` as pass 1 (+ all-reduce under shard.sharded) and one pack per store its consumers
        join at, the float32 tensor from the same pass when some consumer needs it; None when no consumer qualifies."""
        stores, f32 = self._scaled_plan(name, int(op["nb"]), pre.shape)
        if not stores:
            return None
        fn = _abi.FN_QUANTIZED_MAXRELU if op["fn"] == "quantized_maxrelu" else _abi.FN_QUANTIZED_LEAKYMAXRELU
        if fn == _abi.FN_QUANTIZED_LEAKYMAXRELU:
            quantized_ops.check_leaky_alpha(op.get("alpha", quantized_ops.LEAKY_ALPHA), "quantized_leakymaxrelu")
        pre = _abi.require_cuda(pre, op["fn"])
        ws = quantized_ops.maxact_word(pre, None, op["fn"])
        # the float32 tensor comes from the pack's own pass where that streams at full rate (the I8 form); the I4 dual form
        # writes half lines (profiles/scaled/README.md: 650 us against 530 us for the two passes), so there the apply pass
        # runs first and the plain pack after it
        dual = f32 and stores[0] == _abi.STORE_I8
        sc = _Scaled(pre, fn, int(op["nb"]), ws, {}, torch.empty_like(pre) if dual else None, pre.shape)
        if f32 and not dual:
            sc.materialize()
            if self.kernel_log is not None:
                self.kernel_log.append("maxact_apply")
        for j, store in enumerate(stores):
            sc.packs[store] = _abi.maxact_pack(pre, pre.shape[-1], fn, int(op["nb"]), store, ws, sc.f32 if dual and j == 0 else None)
            if self.kernel_log is not None:
                self.kernel_log.append(_abi.last_kernel())
        return sc

    def _pool(self, src, op):
        """A new-form pooling op.  Behind a low-bit clip the activation is packed as its consumers would pack it on load
        and pooled on the codes (the maximum stays packed for the next contraction); everything else is pooled in float32."""
        if isinstance(src, _Virtual) and src.fn in (_abi.FN_BINARY_TANH,) + _abi.QUANT_FNS and src.pre.dim() == 4:
            bits = 1 if src.fn == _abi.FN_BINARY_TANH else src.nb
            store = _abi.STORE_BIN if bits == 1 else _abi.store_for_bits(bits)
            src = _Packed(_abi.pack(src.pre, src.pre.shape[-1], src.fn, bits, store), store, bits, src.pre.shape)
        if isinstance(src, _Packed) and len(src.shape) == 4:
            return _pool_packed(src, op, self.kernel_log)
        y = _GLUE[op["op"]](self._plain(src), op)
        if self.kernel_log is not None:
            self.kernel_log.append(_abi.last_kernel())
        return y

    def _grid_store(self, c):
        """The store at which contraction op `c` reads ternary codes {-1, 0, 1} (_contract), None for float weights."""
        op = self.spec[c]
        wstore = _wstore(op) if op["op"] in ("conv", "dense", "dwconv", "tconv", "gconv") else None
        if wstore is None:
            return None
        if op["kind"] == "ternary" and TERNARY_T2:
            return _abi.STORE_T2             # ternary x ternary: sign / mask planes
        return max(_abi.STORE_I4, wstore if wstore != _abi.STORE_BIN else _abi.STORE_I4)

    def _grid_plan(self, name):
        """The one store every contraction behind ternary activation `name` reads it at, looking through the ops that hand
        packed words on (new-form spatial ops, concats), or None: another consumer, or no common store."""
        stores, todo = set(), [name]
        while todo:
            n = todo.pop()
            if n == self.graph.names[-1]:
                return None
            for c in self.graph.cons.get(n, []):
                op = self.spec[c]
                if op["op"] == "concat" or (op["op"] in _SPATIAL and _new_spatial(op)):
                    todo.append(self.graph.names[c])
                else:
                    stores.add(self._grid_store(c))
        return stores.pop() if len(stores) == 1 else None

    def _pack_clip(self, v, name=None):
        """The unmaterialised clip `v` as the packed codes its consumers would pack on load, or None where it has no
        fixed code (a 16-bit clip) or, for ternary codes, its consumers (those of tensor `name`) share no store."""
        if not isinstance(v, _Virtual) or v.pre.dim() != 4:
            return None
        if v.fn == _abi.FN_GRID:
            store = self._grid_plan(name) if name is not None else None
            if store is None:
                return None
            p = _Packed(_abi.pack(v.materialize(), v.pre.shape[-1], _abi.FN_GRID, 1, store), store, 1, v.pre.shape)
            p.grid = True
            return p
        if v.fn not in (_abi.FN_BINARY_TANH,) + _abi.QUANT_FNS:
            return None
        bits = 1 if v.fn == _abi.FN_BINARY_TANH else v.nb
        store = _abi.STORE_BIN if bits == 1 else _abi.store_for_bits(bits)
        return _Packed(_abi.pack(v.pre, v.pre.shape[-1], v.fn, bits, store), store, bits, v.pre.shape)

    def _spatial(self, src, op, name):
        """A new-form spatial op producing tensor `name`.  Behind a low-bit clip the activation is packed as its consumers
        would pack it on load and moved as codes, which stay packed for the next contraction (ternary codes: on the store
        every contraction behind reads them at).  A pad behind a 1-bit clip (a +-1 code has no zero), an activation
        carried as scaled codes and everything else run in float32."""
        padded = op["op"] == "zeropad"
        if isinstance(src, _Virtual) and not (padded and src.fn == _abi.FN_BINARY_TANH):
            src = self._pack_clip(src, name) or src
        if isinstance(src, _Packed) and len(src.shape) == 4 and not (padded and src.store == _abi.STORE_BIN):
            y, shape = _spatial_run(src.t, src.store, src.bits, src.shape, op, self.kernel_log)
            out = _Packed(y, src.store, src.bits, shape)
            out.grid = src.grid
            return out
        if isinstance(src, _Packed) and self.kernel_log is not None:
            self.kernel_log.append("unpack")
        t = self._plain(src)
        return _spatial_run(t.contiguous(), _abi.STORE_F32, 0, t.shape, op, self.kernel_log)[0]

    def _concat(self, srcs, pack_clips=False):
        """A concat op on the evaluated tensors `srcs` (include/qnn_abi_concat.h).  Packed codes of one store and width
        (the new-form max-pools of two branches) are joined as codes and stay packed for the next contraction.  Clips of
        one function and width that are not materialised yet stay one: concatenation commutes with an elementwise clip,
        so the pre-activations are joined and the consumers still fuse the clip into their pack-on-load.  Everything else
        (a batch-scaled activation included) is materialised and joined in float32.  pack_clips: a branch was resized on
        its codes (_spatial) and meets clips that are not materialised (the skip of an encoder-decoder): those are packed
        as their consumers would pack them on load, so the join stays on codes."""
        if pack_clips and any(isinstance(t, _Packed) for t in srcs):
            like = next(t for t in srcs if isinstance(t, _Packed))
            packs = [t if isinstance(t, _Packed) else None if not isinstance(t, _Virtual) else
                     self._pack_grid_like(t, like) if t.fn == _abi.FN_GRID else self._pack_clip(t) for t in srcs]
            if all(p is not None for p in packs) and len({(p.store, p.bits, p.grid) for p in packs}) == 1:
                srcs = packs
        first = srcs[0]
        if all(isinstance(t, _Packed) for t in srcs) and len({(t.store, t.bits, t.grid) for t in srcs}) == 1:
            shape = _concat_shapes([t.shape for t in srcs])
            y = _concat_run([t.t for t in srcs], [t.shape[-1] for t in srcs], first.store, first.bits,
                            math.prod(shape[:-1]), self.kernel_log)
            out = _Packed(y, first.store, first.bits, shape)
            out.grid = first.grid
            return out
        if all(isinstance(t, _Virtual) for t in srcs) and len({(t.fn, t.nb) for t in srcs}) == 1:
            return _Virtual(_concat_f32([t.pre for t in srcs], self.kernel_log), first.fn, first.nb, first.op)
        return _concat_f32([self._plain(t) for t in srcs], self.kernel_log)

    def _merge(self, srcs, op):
        """A merge op on the evaluated tensors `srcs` (include/qnn_abi_merge.h).  Where every source is packed codes of one
        store, width, meaning (a clip's codes or ternary values) and shape, the op runs on the codes: max / min, and mul
        of +-1 or ternary codes, leave codes that stay packed for the next contraction, the other ops decode in registers
        and leave float32.  A clip that is not materialised yet is packed first, as its consumers would pack it on load.
        Everything else (different stores or widths, ternary values beside a clip's codes, a batch-scaled activation, a
        plain tensor among the sources) is made plain and merged in float32."""
        shape = _merge_shape([t.shape if isinstance(t, (_Packed, _Scaled)) else t.pre.shape if isinstance(t, _Virtual) else t.shape
                              for t in srcs], op)
        packs = [None]
        if all(isinstance(t, (_Packed, _Virtual)) for t in srcs):
            packs = [t if isinstance(t, _Packed) else self._pack_clip(t) for t in srcs]
        if all(p is not None for p in packs) and len({(p.store, p.bits, p.grid) for p in packs}) == 1 and \
                (op["fn"], packs[0].store) not in _MERGE_F32_ROUTE:
            first = packs[0]
            y, out_store = _abi.merge([p.t for p in packs], op["fn"], first.store, first.bits, math.prod(shape[:-1]), shape[-1])
            if self.kernel_log is not None:
                self.kernel_log.append(_abi.last_kernel())
            if out_store == _abi.STORE_F32:
                return y.reshape(shape)
            out = _Packed(y, first.store, first.bits, shape)
            out.grid = first.grid
            return out
        if self.kernel_log is not None and any(isinstance(t, _Packed) for t in srcs):
            self.kernel_log.append("unpack")
        return _merge_f32([self._plain(t) for t in srcs], op, self.kernel_log)

    @staticmethod
    def _pack_grid_like(v, like):
        """Ternary clip `v` packed on the store of `like`, ternary codes themselves; else None."""
        if not like.grid or v.pre.dim() != 4:
            return None
        p = _Packed(_abi.pack(v.materialize(), v.pre.shape[-1], _abi.FN_GRID, 1, like.store), like.store, 1, v.pre.shape)
        p.grid = True
        return p

    def _tail(self, i, src):
        """The classifier tail that starts at avgpool op `i`, fused: (its op indices, result) or None.  The clip in front
        of it is packed as its other consumers pack it on load."""
        t = self.graph.tail_from(i) if self.fuse_tail and isinstance(src, _Virtual) else None
        if t is None or src.fn not in (_abi.FN_BINARY_TANH,) + _abi.QUANT_FNS:
            return None
        end = t[2] if t[3] is None else t[3]
        if end in self.graph.tail_no:
            return None
        bits = 1 if src.fn == _abi.FN_BINARY_TANH else src.nb
        store = _abi.STORE_BIN if bits == 1 else _abi.store_for_bits(bits)
        xp = _Packed(_abi.pack(src.pre, src.pre.shape[-1], src.fn, bits, store), store, bits, src.pre.shape)
        y = self.graph.run_tail(t, xp)
        return None if y is None else (t, y)

    @staticmethod
    def _plain(t):
        if isinstance(t, _Packed):
            return t.to_f32()
        return t.materialize() if isinstance(t, (_Virtual, _Scaled)) else t

    def _contract(self, i, op, src, inv, shift):
        """Conv / dense op `i` on `src` with BN (inv, shift) in its epilogue."""
        kind, wstore, g = op["op"], _wstore(op), self.graph
        if isinstance(src, _Scaled):         # scaled codes: the integer kernels with the word attached, where this op qualified
            store = self._scaled_store(i, src.nb, src.shape)
            if store is not None and store in src.packs:
                w = g.weights(i, store)
                if kind == "conv":
                    N, H, W, _ = src.shape
                    y = _abi.conv2d(w, src.packs[store], store, src.nb, N, H, W, inv, shift, x_scale=src.ws)[0]
                else:
                    y = _abi.dense(w, src.packs[store], store, src.nb, src.shape[0], inv, shift, x_scale=src.ws)
                if self.kernel_log is not None:
                    self.kernel_log.append(_abi.last_kernel())
                return y
        if isinstance(src, _Packed):         # the codes a new-form max-pool, spatial op or concat left
            want = self._grid_store(i) if src.grid else _join_store(src.bits, wstore) if wstore is not None else None
            if wstore is not None and want == src.store and \
                    len(src.shape) == (4 if kind == "conv" else 2):
                w = g.weights(i, src.store)
                if kind == "conv":
                    N, H, W, _ = src.shape
                    return _abi.conv2d(w, src.t, src.store, src.bits, N, H, W, inv, shift)[0]
                return _abi.dense(w, src.t, src.store, src.bits, src.shape[0], inv, shift)
            # another store is needed (or float weights): the values are on the grid, where binary_tanh / quantized_tanh at
            # their width are the identity, so the consumer may clip them again on load
            fn = _abi.FN_GRID if src.grid else _abi.FN_BINARY_TANH if src.store == _abi.STORE_BIN else _abi.FN_QUANTIZED_TANH
            v = _Virtual(src.to_f32(), fn, src.bits, None)
            v._mat = v.pre
            src = v
        if isinstance(src, _Virtual) and wstore is not None:
            bits = 1 if src.fn == _abi.FN_BINARY_TANH else src.nb
            if src.fn == _abi.FN_GRID and op["kind"] == "ternary" and TERNARY_T2:
                store = _abi.STORE_T2        # ternary x ternary: sign / mask planes, two popcounts
            elif src.fn == _abi.FN_GRID:     # ternary codes {-1,0,1}: value = code, needs >= 4 bits
                store = max(_abi.STORE_I4, wstore if wstore != _abi.STORE_BIN else _abi.STORE_I4)
            else:
                store = _join_store(bits, wstore)
            pre = src.pre
            C = pre.shape[-1]
            w = g.weights(i, store)
            nb_in = src.nb if src.fn in _abi.QUANT_FNS else 1
            if kind == "conv" and src.fn == _abi.FN_GRID:
                N, H, W, _ = pre.shape
                xp = _abi.pack(pre, C, _abi.FN_GRID, 1, store)
                return _abi.conv2d(w, xp, store, 1, N, H, W, inv, shift)[0]
            if kind == "conv":
                # activation clip fused on load, BN fused in the epilogue
                return _abi.conv2d_f32in(w, pre, src.fn, nb_in, inv, shift)[0]
            xp = _abi.pack(pre, C, src.fn, nb_in, store)
            return _abi.dense(w, xp, store, bits, pre.shape[0], inv, shift)
        xin = self._plain(src)
        w = g.weights(i, _abi.STORE_F32)
        if kind == "conv":
            N, H, W, _ = xin.shape
            xs = _abi.STORE_U8 if xin.dtype == torch.uint8 else _abi.STORE_F32    # typed image entry
            return _abi.conv2d(w, xin, xs, 0, N, H, W, inv, shift)[0]
        return _abi.dense(w, xin, _abi.STORE_F32, 0, xin.shape[0], inv, shift)

    def _tconv(self, i, op, src):
        """Transposed-convolution op `i` on `src` (include/qnn_abi_tconv.h) under _dwconv's planner rules: (result, index
        of the last op fused into it)."""
        return self._dwconv(i, op, src, run=_abi.tconv)

    def _gconv(self, i, op, src):
        """Grouped-convolution op `i` on `src` (include/qnn_abi_gconv.h) under _dwconv's planner rules: (result, index of
        the last op fused into it)."""
        return self._dwconv(i, op, src, run=_abi.gconv)

    def _dwconv(self, i, op, src, run=None):
        """Depthwise op `i` on `src` (include/qnn_abi_depthwise.h): (result, index of the last op fused into it).  The
        planner rules of a conv: a following BN that is the tensor's only consumer goes into the epilogue, a packed producer
        (codes of the store this op joins at) is read as it is and an unmaterialised clip is packed on load.  Beyond a
        conv, a low-bit clip that alone reads the (BN) output goes into the epilogue too and the result stays packed at
        the clip's width -- the entry has no pack-on-load form, and the 1x1 conv behind a separable block reads the codes.
        A batch-scaled activation is always read as float32 (never as scaled codes)."""
        g, spec, last = self.graph, self.spec, i
        inv = shift = None
        if g.cons.get(g.names[last], []) == [last + 1] and spec[last + 1]["op"] == "bn":
            inv, shift = g.bn[last + 1]
            last += 1
        fn, act_bits, out_store = _abi.FN_NONE, 0, _abi.STORE_F32
        if last + 1 < len(spec) and g.cons.get(g.names[last], []) == [last + 1] and spec[last + 1]["op"] == "act" and \
                _act_code(spec[last + 1]) is not None:
            fn, act_bits = _act_code(spec[last + 1])
            out_store = _abi.STORE_BIN if act_bits == 1 else _abi.store_for_bits(act_bits)
            last += 1
        wstore = _wstore(op)
        xs, xbits, xt = _abi.STORE_F32, 0, None
        if isinstance(src, _Packed):
            want = self._grid_store(i) if src.grid else _join_store(src.bits, wstore) if wstore is not None else None
            if wstore is not None and want == src.store and len(src.shape) == 4:
                xs, xbits, xt = src.store, src.bits, src.t
            else:                            # another store (or float weights): the values are on the grid, clip them again
                cfn = _abi.FN_GRID if src.grid else _abi.FN_BINARY_TANH if src.store == _abi.STORE_BIN else _abi.FN_QUANTIZED_TANH
                v = _Virtual(src.to_f32(), cfn, src.bits, None)
                v._mat = v.pre
                src = v
        if xt is None and isinstance(src, _Virtual) and wstore is not None and src.pre.dim() == 4:
            if src.fn == _abi.FN_GRID:
                xs = self._grid_store(i)
                xbits = 1
                xt = _abi.pack(src.pre, src.pre.shape[-1], _abi.FN_GRID, 1, xs)
            else:
                xbits = 1 if src.fn == _abi.FN_BINARY_TANH else src.nb
                xs = _join_store(xbits, wstore)
                xt = _abi.pack(src.pre, src.pre.shape[-1], src.fn, src.nb if src.fn in _abi.QUANT_FNS else 1, xs)
            if self.kernel_log is not None:
                self.kernel_log.append("pack")
        shape = src.shape if isinstance(src, _Packed) else src.pre.shape if isinstance(src, _Virtual) else None
        if xt is None:
            xt = self._plain(src).contiguous()
            shape = xt.shape
        N, H, W, C = shape
        y, Ho, Wo = (run or _abi.depthwise)(g.weights(i, xs), xt, xs, xbits, N, H, W, inv, shift, fn, act_bits, out_store)
        if self.kernel_log is not None:
            self.kernel_log.append(_abi.last_kernel())
        if out_store != _abi.STORE_F32:
            y = _Packed(y, out_store, act_bits, (N, Ho, Wo, g.weights(i, xs).cout))
        return y, last

    def forward(self, x):
        g, spec = self.graph, self.spec
        env = {"input": _images(x, "GraphModel.forward")}
        skip = set()
        upsampled = set()                    # tensors a tconv or a gconv left as packed codes
        for i, op in enumerate(spec):
            if i in skip:
                continue
            kind, name = op["op"], g.names[i]
            src = env[g.srcs[i][0]]
            fused = self._tail(i, src) if kind == "avgpool" else None
            if fused is not None:
                t, y = fused
                skip.update(k for k in t[1:] if k is not None)      # flatten, dense, softmax: nothing else reads them
                name = g.names[t[2] if t[3] is None else t[3]]
            elif kind in ("conv", "dense"):
                # fuse an immediately following BN that is this tensor's only consumer
                inv = shift = None
                if g.cons.get(name, []) == [i + 1] and spec[i + 1]["op"] == "bn":
                    inv, shift = g.bn[i + 1]
                    skip.add(i + 1)
                    name = g.names[i + 1]
                y = self._contract(i, op, src, inv, shift)
            elif kind in ("dwconv", "tconv", "gconv"):
                y, last = {"dwconv": self._dwconv, "tconv": self._tconv, "gconv": self._gconv}[kind](i, op, src)
                skip.update(range(i + 1, last + 1))
                name = g.names[last]
                if kind in ("tconv", "gconv") and isinstance(y, _Packed):
                    # a decoder's codes, or a grouped 3x3's: the skip they are joined with is packed to meet them
                    upsampled.add(name)
            elif kind == "bn":
                y = _bn_apply(self._plain(src), *g.bn[i])
            elif kind == "add":
                y = _add(self._plain(src), self._plain(env[op["b"]]))
            elif kind == "concat":
                y = self._concat([env[s] for s in g.srcs[i]],
                                 pack_clips=any(s in upsampled or (s in g.prod and spec[g.prod[s]]["op"] in _SPATIAL and
                                                                   _new_spatial(spec[g.prod[s]])) for s in g.srcs[i]))
            elif kind == "merge":
                y = self._merge([env[s] for s in g.srcs[i]], op)
            elif kind in _SPATIAL and _new_spatial(op):
                y = self._spatial(src, op, name)
            elif kind == "act" and _act_code(op) is not None:
                y = _Virtual(self._plain(src), *_act_code(op), op)      # its consumers fuse the clip into their pack-on-load
            elif kind == "act" and self.scaled_codes and op["fn"] in _MAX_ACTS and op["nb"] <= 8:
                pre = self._plain(src)
                y = self._scaled_act(op, pre, name)
                if y is None:                # no consumer qualifies: exactly as without scaled_codes
                    y = _act(pre, op)
            elif kind == "flatten" and isinstance(src, _Scaled) and (self._scaled_flat_ok(i, src.nb, src.shape) or {None}) <= set(src.packs):
                y = src.flat()
            elif kind == "act" and op["fn"] == "ternary_tanh":
                # global mean over the batch tensor: not fusable; the result is on the grid {-1,0,1} and is packed as
                # such by its consumers
                y = _Virtual(_act(self._plain(src), op), _abi.FN_GRID, 1, op)
            elif kind in _POOLS and _new_pool(op):
                y = self._pool(src, op)
            elif kind in _GLUE:
                y = _GLUE[kind](self._plain(src), op)
            else:
                raise ValueError(kind)
            env[name] = y
        return self._plain(env[g.names[-1]])

    __call__ = forward
    predict = forward


# ---------------------------------------------------------------------------
class _Packed:
    """A packed activation tensor: int32 words (pixels, cw) + what the codes mean."""

    grid = False                             # GraphModel: ternary codes {-1, 0, 1} (value = code), not a `bits`-wide clip

    def __init__(self, t, store, bits, shape):
        self.t, self.store, self.bits, self.shape = t, store, bits, tuple(shape)   # shape: NHWC or (N, K)

    def to_f32(self):
        return _abi.unpack(self.t, math.prod(self.shape[:-1]), self.shape[-1], self.store, self.bits).reshape(self.shape)


def _pool_packed(src, op, log=None):
    """A new-form pooling op on the packed NHWC activation `src` (BIN / I4 / I8): the maximum of codes is a code, so
    maxpool / globalmaxpool give a _Packed of the same store and bits; the averages read the codes and give float32."""
    y, shape = _pool_run(src.t, src.store, src.bits, src.shape, op)
    if log is not None:
        log.append(_abi.last_kernel())
    return _Packed(y, src.store, src.bits, shape) if y.dtype == torch.int32 else y


def _ok_lowbit(op):
    """Convs the fused epilogue path takes: low-bit weights (packed input) or the float-input
    first layer; stock float convs stay on the float32 route."""
    return op["op"] == "conv" and op["kind"] in ("binary", "quantized", "ternary") and op.get("nb", 1) <= 8


def _stored_bytes(store, pixels, ch):
    """Bytes of a tensor as stored (SURVEY.md 8d model M1)."""
    if store == _abi.STORE_U8:
        return pixels * ch
    if store in (_abi.STORE_F32, _abi.STORE_F32_IMAGE, _abi.STORE_F32_UNIT):
        return pixels * ch * 4
    return pixels * _abi.words(store, ch) * 4


def _capture_entry(kernel, launch, op, xshape, Ho, Wo, xs, out_store, res, res_store, proj):
    """One launch of a forward as bench.py re-issues it for per-kernel timing (the closure keeps the operands alive);
    bytes = tensors as stored: input + output + shortcut."""
    N, H, W, C = xshape
    kh, kw, _, cout = op["kernel"].shape
    b = _stored_bytes(xs, N * H * W, C) + _stored_bytes(out_store, N * Ho * Wo, cout)
    if res is not None:
        b += _stored_bytes(res_store, N * Ho * Wo, cout)
    if proj is not None:                     # the even rows of the block input (every other pixel of a row shares its
        ps = proj[1].shape                   # 32-byte sectors with the pixels that are read)
        b += _stored_bytes(proj[1].store, ps[0] * ((ps[1] + 1) // 2) * ps[2], ps[3])
    return dict(kernel=kernel, launch=lambda: launch()[0],
                shape=(N, H, W, C, cout, kh, tuple(op.get("strides", (1, 1)))[0],
                       "res_" + ("proj" if proj is not None else "none" if res is None
                                 else "packed" if isinstance(res, _Packed) else "f32")),
                bytes=b, macs=N * Ho * Wo * kh * kw * C * cout, pipe="f32" if kernel.startswith("mfma_f32") else "i8")


class ResidualFusedModel(_DomainFlag):
    """Packed, fused execution of arbitrary (residual) specs -- SURVEY.md 8f.1.

    Every `conv -> BN -> act` chain and every residual merge
    `conv -> BN -> add(shortcut) -> [x0.5] -> act` (models/resnet.py:108-129) is ONE kernel
    launch whose epilogue reads the shortcut (packed codes of the previous activation, or the
    float32 output of the 1x1 projection) and writes the next activation packed.  Evaluation is
    demand-driven from the output so the shortcut operand is always computed before the conv
    that merges it.  The classifier tail AveragePooling2D -> Flatten -> Dense [-> softmax]
    (models/resnet.py:134-140) behind a packed activation is one launch as well (fuse_tail,
    qnn_avgpool_dense_softmax_forward).  Anything else that is not on the low-bit path runs as
    float32 torch ops on unpacked tensors.
    """

    _UNRECOMPUTED = ("ResidualFusedModel: a replayed batch was not image bytes / 255 and has not been "
                     "recomputed on the exact first layer")

    def __init__(self, spec, device="cuda", first_layer="auto", fold=True, fuse_projection=True):
        """first_layer: kernel for float32 images in front of the first (3-channel) conv, as engine.FusedModel:
        "auto" (default: byte kernel with a per-batch domain flag, a batch that is not bytes / 255 is recomputed on the
        exact kernel), "exact" or "image" (float32 bytes / 255 recognised as bytes; domain flag -> check_domain()).  uint8
        images always take the typed QNN_STORE_U8 entry.
        fold: True (default) = every int4 -> int4 layer gets its epilogue folded to integer thresholds the first time it
        runs (qnn_fold_prepare: proven equal to the float32 chain on the layer's whole accumulator domain; layers the
        library cannot fold exactly keep the chain); False = always the float32 chain.  Same bits either way."""
        if first_layer not in ("auto", "exact", "image"):
            raise ValueError("first_layer must be 'auto', 'exact' or 'image', got %r" % (first_layer,))
        _refuse_concat(spec, "ResidualFusedModel")
        _refuse_merge(spec, "ResidualFusedModel")
        _refuse_dwconv(spec, "ResidualFusedModel")
        _refuse_tconv(spec, "ResidualFusedModel")
        _refuse_gconv(spec, "ResidualFusedModel")
        _refuse_spatial(spec, "ResidualFusedModel")
        _refuse_max_acts(spec, "ResidualFusedModel")
        self.first_layer = first_layer
        self.fold = bool(fold)
        self._folds = {}                     # (conv, bn, shortcut kind, ...) -> _abi.Fold or None
        self.fuse_projection = bool(fuse_projection)   # projection shortcuts inside the second conv's launch (qnn_projection_t)
        self._proj_ok = {}                   # conv index -> False once the library had no kernel for the pair
        self.fuse_tail = True                # avg-pool + Flatten + Dense [+ softmax] in one launch (_SpecGraph.run_tail)
        self._plans = {}                     # tensor name -> what _plan() matched in front of it
        self.device = torch.device(device)
        g = self.graph = _SpecGraph(spec, device)
        self.spec, self.names, self.prod, self.srcs, self.cons = spec, g.names, g.prod, g.srcs, g.cons
        self.kernel_log = None
        self.capture = None

    # ---- what the spec alone decides: matched once per model ----------------------
    def _single(self, name, kind):
        """Index of the op producing `name` if it is of `kind` and `name` has one consumer."""
        i = self.prod.get(name)
        if i is None or self.spec[i]["op"] != kind or len(self.cons.get(name, [])) != 1:
            return None
        return i

    def _conv_bn_of(self, name):
        """(conv index, bn index or None) if `name` is conv or conv->bn with single consumers."""
        b = self._single(name, "bn")
        c = self._single(self.srcs[b][0] if b is not None else name, "conv")
        return None if c is None else (c, b)

    def _fusable_before(self, pre):
        """The launches activation input `pre` can be the epilogue of: conv -> bn, or the residual merge
        conv -> bn -> add(shortcut) -> [scale] read with either operand of the add as the main path.
        List of (conv index, bn index or None, shortcut name or None, post_scale); the caller takes the first one whose
        conv it has a kernel for."""
        cb = self._conv_bn_of(pre)
        if cb is not None:
            return [(cb[0], cb[1], None, 1.0)]
        sc_i = self._single(pre, "scale")
        post = float(self.spec[sc_i]["value"]) if sc_i is not None else 1.0
        ad_i = self._single(self.srcs[sc_i][0] if sc_i is not None else pre, "add")
        if ad_i is None:
            return []
        a_n, b_n = self.srcs[ad_i]
        return [cb + (short, post) for main, short in ((b_n, a_n), (a_n, b_n))
                if (cb := self._conv_bn_of(main)) is not None]

    def _projection_of(self, short, ci, fn, bits, out_store):
        """Index of the conv op behind shortcut `short` if it is a projection the second conv `ci` of the block can compute
        inside its own launch (qnn_projection_t, include/qnn_abi.h): a 1x1 strides-2 4-bit QuantizedConv2D with one consumer
        (models/resnet.py:117-124), `ci` a 3x3 stride-1 4-bit layer with cin = cout in {32, 64} = twice the projection's
        input channels, packed 4-bit quantized_tanh output.  None = keep the float32 shortcut tensor."""
        pi = self._single(short, "conv")
        if pi is None:
            return None
        po, mo = self.spec[pi], self.spec[ci]
        pk, mk = po["kernel"].shape, mo["kernel"].shape
        ok = (po.get("kind") == "quantized" and po.get("nb") == 4 and mo.get("kind") == "quantized" and mo.get("nb") == 4
              and tuple(pk[:2]) == (1, 1) and tuple(po.get("strides", (1, 1))) == (2, 2)
              and tuple(mk[:2]) == (3, 3) and tuple(mo.get("strides", (1, 1))) == (1, 1) and mo.get("padding", "same") == "same"
              and _dilation(po) == (1, 1) and _dilation(mo) == (1, 1)
              and mk[2] == mk[3] and mk[3] in (32, 64) and pk[3] == mk[3] and 2 * pk[2] == mk[2]
              and fn == _abi.FN_QUANTIZED_TANH and bits == 4 and out_store == _abi.STORE_I4)
        return pi if ok else None

    def _channels(self, name):
        """Channels of tensor `name` as far as the spec alone says: those of the contraction it descends from through
        the ops that keep them (an add: its first operand), None for the images or behind a flatten."""
        while name in self.prod:
            i = self.prod[name]
            if self.spec[i]["op"] in ("conv", "dense"):
                return int(self.spec[i]["kernel"].shape[-1])
            if self.spec[i]["op"] == "flatten":
                return None
            name = self.srcs[i][0]
        return None

    def _act_out_store(self, name, bits):
        """Packed store the consumers of activation `name` want, or None if one needs float32.  A flatten is looked
        through like a new-form max-pool: it hands the packed words on as they are, so the dense behind it joins the
        store, which is then widened until every pixel's channels fill whole words (the dense weights are packed as one
        contiguous K = H W C vector, as in FusedModel; channels that fill no store's words are unpacked by the flatten)."""
        joins, todo, dense_behind_flatten = [], [(name, False)], False
        while todo:
            n, flat = todo.pop()
            for ci in self.cons.get(n, []):
                op = self.spec[ci]
                if op["op"] in ("conv", "dense") and _wstore(op) is not None:
                    joins.append(_join_store(bits, _wstore(op)))
                    dense_behind_flatten |= flat
                elif op["op"] in ("add", "avgpool", "globalavgpool"):
                    continue             # these read packed codes directly (avgpool: qnn_avgpool_packed_f32 / qnn_pool2d_forward)
                elif op["op"] == "flatten":
                    todo.append((self.names[ci], True))      # the same words, seen as (N, K): what ITS consumers want
                elif op["op"] in ("maxpool", "globalmaxpool") and _new_pool(op):
                    todo.append((self.names[ci], flat))      # codes in, codes out (qnn_pool2d_forward): what ITS consumers want
                else:
                    return None          # (a concat among them: a float32 consumer)
        if not joins:
            return _abi.STORE_BIN if bits == 1 else _abi.store_for_bits(bits)
        if all(j == _abi.STORE_BIN for j in joins):
            store = _abi.STORE_BIN
        else:
            store = max([j for j in joins if j != _abi.STORE_BIN] + [_abi.STORE_I4])
        ch = self._channels(name) if dense_behind_flatten else None
        while ch is not None and ch % _abi.per_word(store) != 0 and store < _abi.STORE_I8:
            store = {_abi.STORE_BIN: _abi.STORE_I4, _abi.STORE_I4: _abi.STORE_I8}[store]
        return store

    def _users_through_pools(self, name):
        """The ops that finally consume tensor `name`, looking through max-pools and flattens (both keep ternary
        codes ternary)."""
        out, todo = [], [name]
        while todo:
            for ci in self.cons.get(todo.pop(), []):
                if self.spec[ci]["op"] in ("maxpool", "globalmaxpool", "flatten"):
                    todo.append(self.names[ci])
                else:
                    out.append(self.spec[ci])
        return out

    def _plan(self, name):
        """What is fused in front of the bn or activation `name`, as far as the spec decides it:
          bn                  (conv, bn) of the launch it is the epilogue of, or None;
          low-bit clip        (packed store or None, output store, the launch out of _fusable_before() or None, the
                              projection conv that launch can compute itself or None);
          LeakyReLU(0.3)      the _fusable_before() list: which one has a kernel depends on the evaluated source;
          ternary_tanh        (packed store or None, every contraction behind it has ternary weights: T2 planes)."""
        if name in self._plans:
            return self._plans[name]
        i = self.prod[name]
        op, pre, p = self.spec[i], self.srcs[i][0], None
        ac = _act_code(op) if op["op"] == "act" else None
        if op["op"] == "bn":
            p = self._conv_bn_of(name)
        elif ac is not None:
            store = self._act_out_store(name, ac[1])
            out_store = store if store is not None else _abi.STORE_F32
            m = next((m for m in self._fusable_before(pre) if _ok_lowbit(self.spec[m[0]])), None)
            pj = self._projection_of(m[2], m[0], ac[0], ac[1], out_store) if m is not None and m[2] is not None else None
            p = store, out_store, m, pj
        elif op["fn"] == "leaky_relu":
            p = self._fusable_before(pre) if F32(op.get("alpha", 0.3)) == F32(0.3) else []
        elif op["fn"] == "ternary_tanh":
            users = self._users_through_pools(name)
            p = (self._act_out_store(name, 4),      # codes {-1,0,1}: at least 4-bit storage
                 any(u["op"] in ("conv", "dense") for u in users) and
                 all(u["op"] in ("add", "avgpool") or (u["op"] in ("conv", "dense") and u["kind"] == "ternary")
                     for u in users))
        self._plans[name] = p
        return p

    def _check_restricted(self):
        for w in self.graph.packed.values():
            if w.shape[2] <= 4 and w.store == _abi.STORE_F32:
                w.check()

    # ---- evaluation: demand-driven from the output, memoised per forward in `memo` (tensor name -> value) ---------
    def _forward(self, x):
        memo = {"input": _images(x, "ResidualFusedModel.forward")}
        res = self._ev(memo, self.names[-1])
        return res.to_f32() if isinstance(res, _Packed) else res

    def _ev(self, memo, name):
        if name not in memo:
            memo[name] = self._compute(memo, self.prod[name], name)
        return memo[name]

    def _f32(self, memo, name):
        v = self._ev(memo, name)
        return v.to_f32() if isinstance(v, _Packed) else v

    def _conv_call(self, memo, ci, bn_i, res, post_scale, fn, bits, out_store, proj=None):
        """Launch conv `ci` with everything fused behind it.  proj = (conv index of a 1x1 strides-2 projection, its packed
        input): the shortcut is computed inside this launch (qnn_projection_t) instead of being read from `res`."""
        op = self.spec[ci]
        src = self._ev(memo, self.srcs[ci][0])
        inv, shift = self.graph.bn[bn_i] if bn_i is not None else (None, None)
        rkw = {}
        if proj is not None:
            psrc = proj[1]
            rkw = dict(post_scale=post_scale,
                       proj=(self.graph.weights(proj[0], psrc.store), psrc.t, psrc.shape[1], psrc.shape[2], psrc.bits))
        if res is not None:
            if isinstance(res, _Packed) and res.store == _abi.STORE_T2:
                res = res.to_f32()           # the shortcut operand of the epilogue reads codes or float32, not bit planes
            if isinstance(res, _Packed):
                rkw = dict(res=res.t, res_store=res.store, res_bits=res.bits, post_scale=post_scale)
            else:
                rkw = dict(res=res.contiguous(), res_store=_abi.STORE_F32, res_bits=0, post_scale=post_scale)
        ab = bits if fn in _abi.QUANT_FNS else 0
        if not isinstance(src, _Packed):
            src = _float_images(src, fn)
        if isinstance(src, _Packed) and _wstore(op) is None:
            src = src.to_f32()               # stock float conv: float32 route
        N, H, W, C = src.shape
        if isinstance(src, _Packed):
            xin, xs, xb = src.t, src.store, src.bits
        else:                                # the images as bytes: typed QNN_STORE_U8 entry
            xin, xs, xb = src.contiguous(), _abi.STORE_U8 if src.dtype == torch.uint8 else _abi.STORE_F32, 0
        w = self.graph.weights(ci, xs if isinstance(src, _Packed) else _abi.STORE_F32)

        dflag = None
        if xs == _abi.STORE_F32 and src is memo["input"] and not self._exact_now and self.first_layer in ("image", "auto"):
            xs = _abi.STORE_F32_IMAGE        # the images: declared as bytes / 255 for this call (typed entry)
            if self.first_layer == "auto":   # ... with the domain-flag word forward() reads to recompute a flagged batch
                dflag = self._own_flag()

        fold = None
        if self.fold and proj is None and w.dilation == (1, 1) and xs == _abi.STORE_I4 and out_store == _abi.STORE_I4 \
                and fn == _abi.FN_QUANTIZED_TANH and ab == 4 \
                and (res is None or (isinstance(res, _Packed) and res.store == _abi.STORE_I4 and res.bits == 4)):
            fkey = (ci, bn_i, xb, None if res is None else float(post_scale))
            if fkey not in self._folds and not torch.cuda.is_current_stream_capturing():
                self._folds[fkey] = _abi.Fold.try_prepare(          # (synchronises: never inside a capture)
                    w, xs, xb, inv, shift, fn, ab, out_store, **rkw)
            fold = self._folds.get(fkey)

        def launch():
            return _abi.conv2d(w, xin, xs, xb, N, H, W, inv, shift, fn, ab, 1, out_store, fold=fold, domain_flag=dflag,
                               **rkw)

        y, Ho, Wo = launch()
        kernel = _abi.last_kernel()
        if self.kernel_log is not None:
            self.kernel_log.append(kernel)
        if self.capture is not None:
            self.capture.append(_capture_entry(kernel, launch, op, (N, H, W, C), Ho, Wo, xs, out_store, res,
                                               rkw.get("res_store"), proj))
        return y if out_store == _abi.STORE_F32 else _Packed(y, out_store, bits, (N, Ho, Wo, op["kernel"].shape[3]))

    def _leaky_on_f32_kernel(self, memo, ci):
        """True if conv `ci` reads float32 activations that only the float32-activation kernel or k_conv_generic take
        (not the images, not 1 or 3 channels): those two implement FN_LEAKY_RELU, so fusing it costs nothing."""
        src = self._ev(memo, self.srcs[ci][0])
        return not isinstance(src, _Packed) and src is not memo["input"] and src.shape[-1] not in (1, 3)

    def _merge(self, memo, m, fn, bits, out_store):
        """Launch `m` out of _fusable_before() with activation `fn` in its epilogue and the shortcut read from its tensor."""
        ci, bn_i, short, post = m
        res = self._ev(memo, short) if short is not None else None
        return self._conv_call(memo, ci, bn_i, res, post, fn, bits, out_store)

    def _activation(self, memo, i, name):
        op, pre_name = self.spec[i], self.srcs[i][0]
        ac = _act_code(op)
        if ac is not None:
            fn, bits = ac
            store, out_store, m, pj = self._plan(name)
            if m is not None and pj is not None and self.fuse_projection and self._proj_ok.get(m[0], True):
                psrc = self._ev(memo, self.srcs[pj][0])
                if isinstance(psrc, _Packed) and psrc.store == _abi.STORE_I4:
                    try:
                        return self._conv_call(memo, m[0], m[1], None, m[3], fn, bits, out_store, proj=(pj, psrc))
                    except _abi.QnnUnsupported:      # no kernel for this pair: two launches, as before
                        self._proj_ok[m[0]] = False
            if m is not None:
                return self._merge(memo, m, fn, bits, out_store)
            pre = self._f32(memo, pre_name)          # no fusable producer: clip (+pack) the float32 tensor
            if store is None:
                return _act(pre, op)
            nb_in = bits if fn in _abi.QUANT_FNS else 1
            return _Packed(_abi.pack(pre, pre.shape[-1], fn, nb_in, store), store, bits, pre.shape)
        if op["fn"] == "leaky_relu":
            # LeakyReLU(alpha = 0.3) inside the launch of the conv behind it, with the float32 shortcut in the epilogue
            m = next((m for m in self._plan(name) if self._leaky_on_f32_kernel(memo, m[0])), None)
            if m is not None:
                return self._merge(memo, m, _abi.FN_LEAKY_RELU, 0, _abi.STORE_F32)
        out = _act(self._f32(memo, pre_name), op)
        if op["fn"] == "ternary_tanh":
            tstore, ternary_users = self._plan(name)
            if TERNARY_T2 and ternary_users:
                tstore = _abi.STORE_T2
            if tstore is not None:
                out = _Packed(_abi.pack(out, out.shape[-1], _abi.FN_GRID, 1, tstore), tstore, 1, out.shape)
        return out

    def _compute(self, memo, i, name):
        op, s0 = self.spec[i], self.srcs[i][0]
        kind = op["op"]
        if kind == "act":
            return self._activation(memo, i, name)
        if kind == "bn":
            cb = self._plan(name)
            if cb is not None:
                return self._conv_call(memo, cb[0], cb[1], None, 1.0, _abi.FN_NONE, 0, _abi.STORE_F32)
            return _bn_apply(self._f32(memo, s0), *self.graph.bn[i])
        if kind == "conv":
            return self._conv_call(memo, i, None, None, 1.0, _abi.FN_NONE, 0, _abi.STORE_F32)
        if kind == "add":
            return _add(self._f32(memo, s0), self._f32(memo, self.srcs[i][1]))
        if kind != "dense" and kind not in _GLUE:
            raise ValueError(kind)
        tail = self.graph.tail(i) if self.fuse_tail and kind in ("dense", "softmax") else None
        if tail is not None:
            # the classifier tail behind a packed activation: one launch; declined (remembered) or not packed: the ops
            # below, one by one, as before
            pooled = self._ev(memo, self.srcs[tail[0]][0])
            y = self.graph.run_tail(tail, pooled) if isinstance(pooled, _Packed) else None
            if y is not None:
                return y
        src = self._ev(memo, s0)
        if isinstance(src, _Packed):         # the ops that read packed words as they are
            if kind == "dense" and _weights_fit(op, src.store):
                return _abi.dense(self.graph.weights(i, src.store), src.t, src.store, src.bits, src.shape[0])
            if kind == "flatten" and src.shape[-1] % _abi.per_word(src.store) == 0:
                return _Packed(src.t, src.store, src.bits, (src.shape[0], math.prod(src.shape[1:])))
            if kind in _POOLS and _new_pool(op):
                if src.store != _abi.STORE_T2 and len(src.shape) == 4:      # on the codes: no float32 copy
                    return _pool_packed(src, op, self.kernel_log)
            elif kind == "avgpool" and src.store != _abi.STORE_T2:   # window sums on the codes: no float32 copy
                return _abi.avgpool_packed(src.t, src.store, src.bits, *src.shape, op.get("size", 8))
        t = src.to_f32() if isinstance(src, _Packed) else src
        if kind == "dense":
            return _abi.dense(self.graph.weights(i, _abi.STORE_F32), t.contiguous(), _abi.STORE_F32, 0, t.shape[0])
        out = _GLUE[kind](t, op)
        if kind in _POOLS and _new_pool(op) and self.kernel_log is not None:
            self.kernel_log.append(_abi.last_kernel())
        if kind in ("maxpool", "globalmaxpool") and isinstance(src, _Packed) and src.store == _abi.STORE_T2:
            # the maximum of ternary codes is a ternary code: stay on the bit planes for the next ternary layer
            out = _Packed(_abi.pack(out.contiguous(), out.shape[-1], _abi.FN_GRID, 1, src.store), src.store, src.bits,
                          out.shape)
        return out


class Pipelined:
    """A model's forward with several batches in flight, without per-layer Python.

    A forward of the fused engines is a handful of short kernels; launched one by one through the Python wrappers the
    GPU waits for the host.  Each of `lanes` lanes owns its intermediate buffers and its own HIP stream, and batches go
    round-robin over the lanes, so one batch's kernel tails and launch boundaries are filled by the next batch's
    kernels (two lanes: +25 % on the headline workload).  Two launch forms:
      * FusedModel (chains): a bound launch plan per lane (FusedModel.bind) -- one foreign call per layer straight on
        the caller's batch and into the caller's result tensor: nothing is copied;
      * every other engine (130 launches per ResNet forward): a hipGraph of model(x) per lane; batches are copied into
        the lane's static input and the logits out of its static output on the lane's stream.
    Nothing synchronises the host until the caller asks for the result.  lanes_for() hands out the hipGraph lanes
    (bench.py's timed region replays them on inputs already resident in the lanes' static buffers).

        pipe = engine.Pipelined(model, lanes=2)
        logits = pipe(images)            # CUDA tensor (N, H, W, C), float32 or uint8, any N -> (N, classes)

    Networks whose result depends on the batch composition (ternary_tanh thresholds at the batch mean) are still
    correct: every replay sees exactly one full batch, the ragged tail runs eagerly.
    """

    def __init__(self, model, lanes=2, batch_size=4096):
        if lanes < 1:
            raise ValueError("lanes must be >= 1")
        self.model, self.nlanes, self.batch_size = model, int(lanes), int(batch_size)
        self._lanes = {}                     # (batch shape, dtype) -> list of lane dicts

    def _auto(self, example):
        """True if batches like `example` run the model's "auto" first layer (float32 images, per-batch domain flags)."""
        return getattr(self.model, "first_layer", None) == "auto" and example.dtype == torch.float32

    def _capture(self, example, slots=1, inputs=1):
        key = (tuple(example.shape), example.dtype, slots, inputs)
        if key in self._lanes:
            return self._lanes[key]
        lanes = []
        cur = torch.cuda.current_stream()
        direct = slots > 1 and isinstance(self.model, FusedModel) and not self.model.steps[-1]["softmax"]
        auto = self._auto(example)
        for _ in range(self.nlanes):
            xs = torch.empty_like(example)
            xs.copy_(example)
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                for _ in range(2):           # warm-up outside capture: lazy initialisation, allocator pools, folds
                    y0 = self.model(xs)
            cur.wait_stream(side)
            lane = dict(stream=torch.cuda.Stream(), x=xs)
            if auto:
                # "auto" first layer: every lane owns the domain-flag word its graphs write (the model's word while the
                # lane is captured); forward() copies it out per batch, bench.py reads it after its timed region
                lane["flag"] = torch.zeros(1, dtype=torch.int32, device=example.device)
            with self.model.flag_word(lane["flag"]) if auto else contextlib.nullcontext():
                self._capture_lane(lane, xs, y0, example, slots, inputs, direct)
            lanes.append(lane)
        torch.cuda.synchronize()
        self._lanes[key] = lanes
        return lanes

    def _capture_lane(self, lane, xs, y0, example, slots, inputs, direct):
        """Capture the graphs of one lane on its static input `xs` (y0: what the warm-up forward returned)."""
        if slots == 1 and inputs > 1:
            # `inputs` static input buffers per lane, one graph each: a replay loop that rotates them streams its
            # images from HBM instead of re-reading one batch out of the 256 MB Infinity Cache (bench.py)
            lane.update(xs=[xs] + [xs.clone() for _ in range(inputs - 1)], graphs=[], ys=[])
            for xi in lane["xs"]:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    yi = self.model(xi)
                lane["graphs"].append(g)
                lane["ys"].append(yi)
            lane.update(graph=lane["graphs"][0], y=lane["ys"][0])
        elif slots == 1:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                ys = self.model(xs)
            lane.update(graph=g, y=ys)
        else:
            # `slots` result slots per lane (a ring the caller hands to one collective per `slots` batches): one
            # graph per slot whose last kernel writes straight into the slot -- or, for engines that cannot be told
            # where to write, ONE graph plus a copy into the slot after every replay
            B = y0.shape[0]
            ring = torch.zeros((slots * B,) + tuple(y0.shape[1:]), dtype=y0.dtype, device=y0.device)
            lane.update(ring=ring, direct=direct, graphs=[])
            N, H, W, _ = example.shape
            # `inputs` static input buffers: slot j's graph reads buffer j % inputs (HBM-streaming replays, as above)
            lane["xs"] = [xs] + [xs.clone() for _ in range(min(inputs, slots if direct else 1) - 1)]
            for j in range(slots if direct else 1):
                xi = lane["xs"][j % len(lane["xs"])]
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    if direct:
                        ys = self.model.forward_from(0, xi, N, H, W, out=ring[j * B:(j + 1) * B])
                    else:
                        ys = self.model(xi)
                lane["graphs"].append(g)
            lane.update(graph=lane["graphs"][0], y=ys)

    def lanes_for(self, example, slots=1, inputs=1):
        """The captured lanes for batches shaped like `example` (bench.py replays them directly).  slots > 1: every
        lane owns a ring of `slots` result blocks (`ring`, `graphs`, `direct`): replay `graphs[j]` to fill slot j when
        `direct`, else replay `graph` and copy `y` into the slot.  inputs > 1: `xs` = that many static input buffers per
        lane (fill them with distinct batches), `graphs[j]` reads `xs[j % inputs]`.  "auto" first layer: `flag` = the
        lane's domain-flag word (see lane_flags_raised)."""
        return self._capture(example, slots, inputs)

    def lane_flags_raised(self):
        """Synchronise; True (and clear) if any captured lane's "auto" domain flag is raised: some replayed batch was not
        image bytes / 255 and -- replayed by hand rather than through forward() -- has not been recomputed."""
        torch.cuda.synchronize()
        raised = False
        for lanes in self._lanes.values():
            for ln in (lanes or []):
                f = ln.get("flag")
                if f is not None and int(f.item()) != 0:
                    f.zero_()
                    raised = True
        return raised

    def _bound_lanes(self, example):
        """Zero-copy form for FusedModel: per lane a bound launch plan (FusedModel.bind) with its own intermediate
        tensors.  A hipGraph bakes its kernel arguments in, so replaying the first layer from a graph would mean copying
        every batch into a static input first (50 MB per 4096 float32 CIFAR images, a third of the headline's time);
        the plan launches the same kernels directly on the caller's batch and into the caller's result, one foreign
        call per layer."""
        key = ("bound", tuple(example.shape), example.dtype)
        if key not in self._lanes:
            lanes = []
            for _ in range(self.nlanes):
                b = self.model.bind(example)
                if b is None:
                    lanes = None
                    break
                lanes.append(dict(stream=torch.cuda.Stream(), plan=b[0], yshape=b[1], ydtype=b[2]))
            torch.cuda.synchronize()
            self._lanes[key] = lanes
        return self._lanes[key]

    def _forward_zero_copy(self, x, B, nfull, lanes):
        m = self.model
        outs = torch.empty((x.shape[0],) + lanes[0]["yshape"][1:], dtype=lanes[0]["ydtype"], device=x.device)
        cur = torch.cuda.current_stream()
        auto = self._auto(x)
        flags = torch.zeros(nfull, dtype=torch.int32, device=x.device) if auto else None    # one domain-flag word per batch
        for ln in lanes:
            ln["stream"].wait_stream(cur)
        xb, xs = x.data_ptr(), B * x.stride(0) * x.element_size()
        yb, ys = outs.data_ptr(), B * outs.stride(0) * outs.element_size()
        fb = flags.data_ptr() if auto else 0
        for i in range(nfull):
            ln = lanes[i % len(lanes)]
            if auto:
                ln["plan"](ln["stream"].cuda_stream, xb + i * xs, yb + i * ys, fb + 4 * i)
            else:
                ln["plan"](ln["stream"].cuda_stream, xb + i * xs, yb + i * ys)
        for ln in lanes:
            cur.wait_stream(ln["stream"])
        if auto:
            self._recompute_flagged(x, outs, B, flags)
        return outs

    def _recompute_flagged(self, x, outs, B, flags):
        """"auto" first layer: the batches whose domain flag is raised (not image bytes / 255) are recomputed on the exact
        first layer, in place.  One host synchronisation (the flags are read)."""
        for i in torch.nonzero(flags).flatten().tolist():
            outs[i * B:(i + 1) * B] = self.model.forward_exact(x[i * B:(i + 1) * B])

    def forward(self, x):
        x = _images(x, "Pipelined.forward")
        N = x.shape[0]
        B = min(self.batch_size, N)
        nfull = N // B if B else 0
        outs = None
        cur = torch.cuda.current_stream()
        bound = self._bound_lanes(x[:B]) if (nfull and isinstance(self.model, FusedModel)) else None
        if bound:
            outs = self._forward_zero_copy(x, B, nfull, bound)
        elif nfull:
            lanes = self._capture(x[:B])
            outs = torch.empty((N,) + tuple(lanes[0]["y"].shape[1:]), dtype=lanes[0]["y"].dtype, device=x.device)
            auto = self._auto(x)
            flags = torch.zeros(nfull, dtype=torch.int32, device=x.device) if auto else None
            for ln in lanes:
                ln["stream"].wait_stream(cur)          # x was produced on the caller's stream
            for i in range(nfull):
                ln = lanes[i % len(lanes)]
                with torch.cuda.stream(ln["stream"]):
                    ln["x"].copy_(x[i * B:(i + 1) * B], non_blocking=True)
                    ln["graph"].replay()
                    outs[i * B:(i + 1) * B].copy_(ln["y"], non_blocking=True)
                    if auto:                           # this batch's flag out of the lane's word, which is cleared
                        flags[i:i + 1].copy_(ln["flag"], non_blocking=True)
                        ln["flag"].zero_()
            for ln in lanes:
                cur.wait_stream(ln["stream"])
            if auto:
                self._recompute_flagged(x, outs, B, flags)
        if nfull * B < N:                              # ragged tail: eager, its own batch
            tail = self.model(x[nfull * B:])
            if outs is None:
                return tail
            outs[nfull * B:] = tail
        return outs

    __call__ = forward
    predict = forward

    def check_domain(self):
        """Raise QnnError if a restricted-domain first layer met inputs outside its domain that nobody recomputed
        ("image" / "fixed": the layer's flag; "auto": a lane flag left by hand-driven graph replays)."""
        if self.lane_flags_raised():
            raise _abi.QnnError("Pipelined: a replayed batch was not image bytes / 255 and has not been recomputed on the "
                                "exact first layer (drive the batches through forward())")
        if hasattr(self.model, "check_domain"):
            self.model.check_domain()
        else:
            torch.cuda.synchronize()

    def clear(self):
        """Release every captured lane (graphs, static inputs, intermediate tensors)."""
        self._lanes.clear()


# ---------------------------------------------------------------------------
class LayerModel:
    """The spec instantiated as Keras-compatible layer objects, called one by one
    (every low-bit layer: float32 NHWC in -> float32 NHWC out)."""

    def __init__(self, spec, device="cuda", fuse_input_activation=True):
        _refuse_concat(spec, "LayerModel")
        self.device = torch.device(device)
        self.spec = spec
        self.layers = {}
        self.graph = _SpecGraph(spec, device)
        prev_act = {}
        for i, op in enumerate(spec):
            if op["op"] not in ("conv", "dense", "dwconv", "tconv", "gconv"):
                continue
            kw = dict(use_bias=op.get("bias") is not None, device=device)
            if op["op"] == "gconv":
                kh, kw_, cg, cout = op["kernel"].shape
                groups = int(op.get("groups", 1))
                kw.update(strides=tuple(op.get("strides", (1, 1))), padding=op.get("padding", "same"),
                          dilation_rate=_dilation(op), groups=groups)
                H = float(op.get("H", 1.0))
                if op["kind"] == "binary":
                    layer = BinaryGroupedConv2D(cout, (kh, kw_), H=H, **kw)
                elif op["kind"] == "quantized":
                    layer = QuantizedGroupedConv2D(cout, (kh, kw_), H=H, nb=op["nb"], **kw)
                elif op["kind"] == "ternary":
                    layer = TernaryGroupedConv2D(cout, (kh, kw_), H=H, **kw)
                else:
                    layer = GroupedConv2D(cout, (kh, kw_), **kw)
                layer.build((None, None, None, cg * groups))
                ws = [op["kernel"]] + ([op["bias"]] if op.get("bias") is not None else [])
                layer.set_weights(ws)
                self.layers[i] = layer
                continue
            if op["op"] == "tconv":
                kh, kw_, cout, cin = op["kernel"].shape
                kw.update(strides=tuple(op.get("strides", (1, 1))), padding=op.get("padding", "same"))
                H = float(op.get("H", 1.0))
                if op["kind"] == "binary":
                    layer = BinaryConv2DTranspose(cout, (kh, kw_), H=H, **kw)
                elif op["kind"] == "quantized":
                    layer = QuantizedConv2DTranspose(cout, (kh, kw_), H=H, nb=op["nb"], **kw)
                elif op["kind"] == "ternary":
                    layer = TernaryConv2DTranspose(cout, (kh, kw_), H=H, **kw)
                else:
                    layer = Conv2DTranspose(cout, (kh, kw_), **kw)
                layer.build((None, None, None, cin))
                ws = [op["kernel"]] + ([op["bias"]] if op.get("bias") is not None else [])
                layer.set_weights(ws)
                self.layers[i] = layer
                continue
            if op["op"] == "dwconv":
                kh, kw_, cin, M = op["kernel"].shape
                kw.update(strides=tuple(op.get("strides", (1, 1))), padding=op.get("padding", "same"),
                          dilation_rate=_dilation(op), depth_multiplier=int(op.get("depth_multiplier", M)))
                H = float(op.get("H", 1.0))
                if op["kind"] == "binary":
                    layer = BinaryDepthwiseConv2D((kh, kw_), H=H, **kw)
                elif op["kind"] == "quantized":
                    layer = QuantizedDepthwiseConv2D((kh, kw_), H=H, nb=op["nb"], **kw)
                elif op["kind"] == "ternary":
                    layer = TernaryDepthwiseConv2D((kh, kw_), H=H, **kw)
                else:
                    layer = DepthwiseConv2D((kh, kw_), **kw)
                layer.build((None, None, None, cin))
            elif op["op"] == "conv":
                kh, kw_, cin, cout = op["kernel"].shape
                kw.update(kernel_size=(kh, kw_), strides=tuple(op.get("strides", (1, 1))),
                          padding=op.get("padding", "same"), dilation_rate=_dilation(op))
                if op["kind"] == "binary":
                    layer = BinaryConv2D(cout, H=1., **kw)
                elif op["kind"] == "quantized":
                    layer = QuantizedConv2D(cout, H=1., nb=op["nb"], **kw)
                elif op["kind"] == "ternary":
                    layer = TernaryConv2D(cout, H=1., **kw)
                else:
                    raise _abi.QnnError("LayerModel covers the low-bit layers only")
                layer.build((None, None, None, cin))
            else:
                cin, cout = op["kernel"].shape
                if op["kind"] == "binary":
                    layer = BinaryDense(cout, **kw)
                elif op["kind"] == "quantized":
                    layer = QuantizedDense(cout, nb=op["nb"], **kw)
                elif op["kind"] == "ternary":
                    layer = TernaryDense(cout, **kw)
                else:
                    raise _abi.QnnError("LayerModel covers the low-bit layers only")
                layer.build((None, cin))
            ws = [op["kernel"]] + ([op["bias"]] if op.get("bias") is not None else [])
            layer.set_weights(ws)
            self.layers[i] = layer
        self.fuse_input_activation = fuse_input_activation


    @staticmethod
    def _grid(op):
        """What a layer may assume about the values activation `op` hands it (layers/_base.py, input_domain)."""
        if op["fn"] in _QUANT_ACTS:          # all three leave values k / 2^(nb-1)
            return ("quantized", op["nb"]) if op["nb"] <= 8 else None
        return {"binary_tanh": "binary", "ternary_tanh": ("quantized", 1)}.get(op["fn"])      # grid {-1,0,1}: value = code

    def forward(self, x, upto=None):
        """upto: index of a spec op whose output is returned instead of the network's (the intermediate model of
        test_resnet.py:70-72, `Model(inputs=model.input, outputs=model.get_layer(name).output)`)."""
        x = _abi.require_cuda(x, "LayerModel.forward")
        g = self.graph
        env = {"input": x}
        dom = {"input": None}     # what is known about each tensor's values
        for i, op in enumerate(self.spec):
            kind, sname = op["op"], g.srcs[i][0]
            src, d = env[sname], None
            if kind == "add":
                y = _add(src, env[op["b"]])
            elif kind == "merge":
                y = _merge_f32([env[s] for s in g.srcs[i]], op)
            elif kind in ("conv", "dense", "dwconv", "tconv", "gconv"):
                layer = self.layers[i]
                layer.input_domain = dom.get(sname) if self.fuse_input_activation else None
                y = layer(src)
            elif kind == "bn":
                y = _bn_apply(src, *g.bn[i])
            elif kind in _GLUE:
                y = _GLUE[kind](src, op)
                if kind == "act":
                    d = self._grid(op)
                elif kind in ("maxpool", "globalmaxpool", "flatten", "crop", "upsample"):
                    d = dom.get(sname)      # max of grid values stays on the grid; a copy of pixels does too
            else:
                raise ValueError(kind)
            env[g.names[i]] = y
            dom[g.names[i]] = d
            if upto is not None and i == upto:
                return y
        return env[g.names[-1]]

    __call__ = forward
    predict = forward
