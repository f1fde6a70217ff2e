"""ctypes binding of include/qnn_abi.h, qnn_abi_dilation.h, qnn_abi_qact.h, qnn_abi_maxact.h, qnn_abi_pool.h,
qnn_abi_scaled.h, qnn_abi_concat.h, qnn_abi_spatial.h, qnn_abi_depthwise.h, qnn_abi_tconv.h, qnn_abi_gconv.h and
qnn_abi_merge.h (csrc/libqnn_hip.so).

The library is loaded eagerly and loudly: a missing or unloadable .so raises at
import time of any op that needs it (there is no CPU implementation to fall back
to).  Tensors cross the boundary as raw device pointers (``tensor.data_ptr()``)
plus the current HIP stream of torch.
"""
import ctypes
import numbers
import os

import torch

from . import _build

QNN_OK = 0
QNN_EUNSUPPORTED = -2
STORE_F32, STORE_BIN, STORE_T2, STORE_I4, STORE_I8, STORE_U8 = 0, 1, 2, 4, 8, 16
STORE_F32_IMAGE, STORE_F32_UNIT = 17, 18      # float32 input with a declared domain (first layer; qnn_abi.h)
W_FLOAT, W_BINARY, W_QUANT, W_TERNARY = 0, 1, 2, 3
FN_NONE, FN_BINARY_TANH, FN_QUANTIZED_TANH, FN_TERNARY_TANH, FN_GRID = 0, 1, 2, 3, 4
FN_LEAKY_RELU = 5                   # Keras LeakyReLU() at alpha = float32(0.3), float32 output only
# quantized_ops.py:69-84 / 102-123 (alpha = float32(0.1)): codes on quantized_tanh's grid, accepted wherever it is except
# by the folds, the fused conv + classifier entry and a QNN_STORE_U8 input (qnn_abi.h)
FN_QUANTIZED_RELU, FN_QUANTIZED_LEAKYRELU = 6, 7
QUANT_FNS = (FN_QUANTIZED_TANH, FN_QUANTIZED_RELU, FN_QUANTIZED_LEAKYRELU)      # the activations that carry act_bits
# quantized_ops.py:125-171 (include/qnn_abi_maxact.h): scaled by the batch tensor's maximum, so NOT in QUANT_FNS -- only the
# elementwise entry qnn_quantized_maxact_f32 takes them, every conv / dense / pack / fold entry answers QNN_EUNSUPPORTED
FN_QUANTIZED_MAXRELU, FN_QUANTIZED_LEAKYMAXRELU = 8, 9
MAXACT_FNS = (FN_QUANTIZED_MAXRELU, FN_QUANTIZED_LEAKYMAXRELU)

EXPORTS = [
    "qnn_version", "qnn_last_error", "qnn_last_kernel", "qnn_set_conv_impl",
    "qnn_binary_tanh_f32", "qnn_quantized_tanh_f32", "qnn_ternary_tanh_f32",
    "qnn_ternary_abs_sum_f32", "qnn_ternary_apply_f32",
    "qnn_packed_bytes", "qnn_pack_f32", "qnn_unpack_f32", "qnn_avgpool_packed_f32", "qnn_softmax_f32",
    "qnn_prepack_weights", "qnn_free_weights", "qnn_weights_dequant", "qnn_weights_check",
    "qnn_conv2d_forward", "qnn_dense_forward", "qnn_conv2d_forward_f32in", "qnn_conv2d_workspace_bytes",
    "qnn_conv2d_dense_forward", "qnn_avgpool_dense_softmax_forward",
    "qnn_fold_prepare", "qnn_fold_free", "qnn_fold_info", "qnn_fold_constants", "qnn_fold_eval",
]


# include/qnn_abi_dilation.h: the extension header of ABI 4 (qnn_abi.h and its symbol list are unchanged)
EXPORTS_DILATION = ["qnn_prepack_weights_dilated"]

# include/qnn_abi_qact.h: the quantised activations as an elementwise op, an extension header of the same kind
EXPORTS_QACT = ["qnn_quantized_act_f32"]

# include/qnn_abi_maxact.h: quantized_maxrelu / quantized_leakymaxrelu as a reduction, an apply pass and the two in sequence
EXPORTS_MAXACT = ["qnn_maxact_max_f32", "qnn_maxact_apply_f32", "qnn_quantized_maxact_f32"]

# include/qnn_abi_pool.h: MaxPooling2D / AveragePooling2D with pool_size, strides and padding, on float32 and on packed codes
EXPORTS_POOL = ["qnn_pool2d_out_hw", "qnn_pool2d_forward"]
POOL_MAX, POOL_AVG = 0, 1

# include/qnn_abi_scaled.h: the two activations of qnn_abi_maxact.h as packed codes plus the device-resident scale, and the
# conv / dense entries that consume them
EXPORTS_SCALED = ["qnn_maxact_pack_f32", "qnn_conv2d_forward_scaled", "qnn_dense_forward_scaled"]

# include/qnn_abi_concat.h: Concatenate(axis=-1) on float32 and on packed codes
EXPORTS_CONCAT = ["qnn_concat_forward"]
CONCAT_MAX = 8

# include/qnn_abi_spatial.h: Cropping2D / UpSampling2D (nearest) / ZeroPadding2D on float32 and on packed codes
EXPORTS_SPATIAL = ["qnn_spatial2d_out_hw", "qnn_spatial2d_forward"]

# include/qnn_abi_depthwise.h: DepthwiseConv2D with float / binary / quantized / ternary weights on float32 and packed codes
EXPORTS_DEPTHWISE = ["qnn_depthwise_prepack", "qnn_depthwise_free", "qnn_depthwise_dequant", "qnn_depthwise_out_hw",
                     "qnn_depthwise_forward"]
DW_MAX_WINDOW = 7

# include/qnn_abi_tconv.h: Conv2DTranspose with float / binary / quantized / ternary weights on float32 and packed codes
EXPORTS_TCONV = ["qnn_tconv_prepack", "qnn_tconv_free", "qnn_tconv_dequant", "qnn_tconv_out_hw", "qnn_tconv_forward"]
TC_MAX_WINDOW, TC_MAX_STRIDE = 8, 4

# include/qnn_abi_gconv.h: Conv2D(groups=g) with float / binary / quantized / ternary weights on float32 and packed codes
EXPORTS_GCONV = ["qnn_gconv_prepack", "qnn_gconv_free", "qnn_gconv_dequant", "qnn_gconv_out_hw", "qnn_gconv_forward"]
GC_MAX_WINDOW = 7

# include/qnn_abi_merge.h: Add / Subtract / Multiply / Average / Maximum / Minimum on float32 and on packed codes
EXPORTS_MERGE = ["qnn_merge_out_store", "qnn_merge_forward"]
MERGE_MAX = 8
MERGE_ADD, MERGE_SUB, MERGE_MUL, MERGE_AVG, MERGE_MAXIMUM, MERGE_MINIMUM = range(6)
MERGE_OPS = {"add": MERGE_ADD, "sub": MERGE_SUB, "mul": MERGE_MUL, "avg": MERGE_AVG, "max": MERGE_MAXIMUM, "min": MERGE_MINIMUM}


class Spatial2D(ctypes.Structure):
    """qnn_spatial2d_t"""
    _fields_ = [("crop", ctypes.c_int32 * 4), ("up", ctypes.c_int32 * 2), ("pad", ctypes.c_int32 * 4)]


class Merge(ctypes.Structure):
    """qnn_merge_t"""
    _fields_ = [("n", ctypes.c_int32), ("op", ctypes.c_int32), ("x", ctypes.c_void_p * MERGE_MAX)]


class Concat(ctypes.Structure):
    """qnn_concat_t"""
    _fields_ = [("n", ctypes.c_int32), ("channels", ctypes.c_int32 * CONCAT_MAX), ("x", ctypes.c_void_p * CONCAT_MAX)]


class Pool2D(ctypes.Structure):
    """qnn_pool2d_t"""
    _fields_ = [("mode", ctypes.c_int32), ("ph", ctypes.c_int32), ("pw", ctypes.c_int32), ("sh", ctypes.c_int32),
                ("sw", ctypes.c_int32), ("same_pad", ctypes.c_int32)]


class Projection(ctypes.Structure):
    """qnn_projection_t: the shortcut as a 1x1 strides-2 convolution of the block input, computed inside the launch."""
    _fields_ = [("w", ctypes.c_void_p), ("x", ctypes.c_void_p), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("x_bits", ctypes.c_int32)]


class Epilogue(ctypes.Structure):
    _fields_ = [("bn_inv", ctypes.c_void_p), ("bn_shift", ctypes.c_void_p),
                ("fn", ctypes.c_int32), ("act_bits", ctypes.c_int32),
                ("pool", ctypes.c_int32), ("out_store", ctypes.c_int32),
                ("res", ctypes.c_void_p), ("res_store", ctypes.c_int32), ("res_bits", ctypes.c_int32),
                ("post_scale", ctypes.c_float), ("trick_c", ctypes.c_float), ("trick_s", ctypes.c_float),
                ("fold", ctypes.c_void_p), ("flags", ctypes.c_uint32), ("domain_flag", ctypes.c_void_p),
                ("proj", ctypes.c_void_p)]


class FoldInfo(ctypes.Structure):
    _fields_ = [("channels", ctypes.c_int32), ("folded", ctypes.c_int32), ("usable", ctypes.c_int32),
                ("shortcut_codes", ctypes.c_int32), ("points", ctypes.c_int64),
                ("acc_lo", ctypes.c_int32), ("acc_hi", ctypes.c_int32), ("mode", ctypes.c_int32)]


class QnnError(RuntimeError):
    pass


class QnnUnsupported(QnnError):
    """QNN_EUNSUPPORTED from an optional fused form (a projection shortcut computed inside the launch, the classifier tail
    in one launch): the caller keeps the form it had."""


class NotFusable(QnnError):
    """A net spec that engine.FusedModel cannot express as one packed chain (the caller picks another
    engine).  Every other failure -- prepack, out of memory, a planner bug -- stays a plain QnnError."""


_lib = None


def lib_path():
    # QNN_LIB: an alternative build of the same ABI (tools/build_variant.py, A/B kernel experiments only)
    return os.environ.get("QNN_LIB") or _build.LIB


def load():
    """Return the loaded library; raise if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise QnnError(
            "libqnn_hip.so is not built (%s). Run `python -c \"import __graft_entry__ as g; "
            "g.build()\"` (needs hipcc). There is no CPU fallback." % path)
    if path == _build.LIB and _build.built_hash() != _build.source_hash() and os.environ.get("QNN_ALLOW_STALE_LIB") != "1":
        raise QnnError(
            "libqnn_hip.so was built from other sources than the ones in csrc/ (stamp %s, sources %s). Rebuild: "
            "`python -c \"import __graft_entry__ as g; g.build()\"`." % (_build.built_hash(), _build.source_hash()))
    lib = ctypes.CDLL(path)
    vp, ci, sz, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
    lib.qnn_version.restype = ci
    lib.qnn_last_error.restype = ctypes.c_char_p
    lib.qnn_last_kernel.restype = ctypes.c_char_p
    lib.qnn_set_conv_impl.argtypes = [ci]
    lib.qnn_binary_tanh_f32.argtypes = [vp, vp, sz, vp]
    lib.qnn_quantized_tanh_f32.argtypes = [vp, vp, sz, ci, vp]
    lib.qnn_quantized_act_f32.argtypes = [vp, vp, sz, ci, ci, vp]
    lib.qnn_maxact_max_f32.argtypes = [vp, sz, vp, vp]
    lib.qnn_maxact_apply_f32.argtypes = [vp, vp, sz, ci, ci, vp, vp]
    lib.qnn_quantized_maxact_f32.argtypes = [vp, vp, sz, ci, ci, vp, vp]
    lib.qnn_ternary_tanh_f32.argtypes = [vp, vp, sz, vp, vp]
    lib.qnn_ternary_abs_sum_f32.argtypes = [vp, sz, vp, vp]
    lib.qnn_ternary_apply_f32.argtypes = [vp, vp, sz, vp, vp]
    lib.qnn_packed_bytes.argtypes = [ci, sz, ci]
    lib.qnn_packed_bytes.restype = sz
    lib.qnn_pack_f32.argtypes = [vp, vp, sz, ci, ci, ci, ci, vp]
    lib.qnn_unpack_f32.argtypes = [vp, vp, sz, ci, ci, ci, vp]
    lib.qnn_avgpool_packed_f32.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, vp, vp]
    lib.qnn_softmax_f32.argtypes = [vp, vp, ctypes.c_size_t, ci, vp]
    lib.qnn_prepack_weights.argtypes = [ci, ci, fl, vp, ci, ci, ci, ci, vp, ci, ci, ci, vp,
                                        ctypes.POINTER(vp)]
    lib.qnn_prepack_weights_dilated.argtypes = [ci, ci, fl, vp, ci, ci, ci, ci, vp, ci, ci, ci, ci, ci, vp,
                                                ctypes.POINTER(vp)]
    lib.qnn_free_weights.argtypes = [vp]
    lib.qnn_weights_dequant.argtypes = [vp, vp, vp]
    lib.qnn_weights_check.argtypes = [vp, vp]
    lib.qnn_conv2d_forward.argtypes = [vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(Epilogue), vp, vp]
    lib.qnn_dense_forward.argtypes = [vp, vp, ci, ci, ci, ctypes.POINTER(Epilogue), vp, vp]
    lib.qnn_conv2d_dense_forward.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(Epilogue),
                                             ctypes.POINTER(Epilogue), vp, vp]
    lib.qnn_avgpool_dense_softmax_forward.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, ctypes.POINTER(Epilogue), ci, vp,
                                                      vp, vp]
    lib.qnn_fold_prepare.argtypes = [vp, ci, ci, ctypes.POINTER(Epilogue), vp, ctypes.POINTER(vp)]
    lib.qnn_fold_free.argtypes = [vp]
    lib.qnn_fold_info.argtypes = [vp, ctypes.POINTER(FoldInfo)]
    lib.qnn_fold_constants.argtypes = [vp, vp, vp, vp, vp]
    lib.qnn_fold_eval.argtypes = [vp, ci, vp, vp, vp, sz, vp]
    lib.qnn_conv2d_workspace_bytes.argtypes = [vp, ci, ci, ci]
    lib.qnn_conv2d_workspace_bytes.restype = sz
    lib.qnn_conv2d_forward_f32in.argtypes = [vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(Epilogue), vp,
                                             vp, sz, vp]
    lib.qnn_pool2d_out_hw.argtypes = [ci, ci, ctypes.POINTER(Pool2D), ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.qnn_pool2d_forward.argtypes = [vp, ci, ci, ci, ci, ci, ci, ctypes.POINTER(Pool2D), vp, ci, vp]
    lib.qnn_maxact_pack_f32.argtypes = [vp, vp, vp, sz, ci, ci, ci, ci, vp, vp]
    lib.qnn_conv2d_forward_scaled.argtypes = [vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(Epilogue), vp, vp, vp]
    lib.qnn_dense_forward_scaled.argtypes = [vp, vp, ci, ci, ci, ctypes.POINTER(Epilogue), vp, vp, vp]
    lib.qnn_concat_forward.argtypes = [ctypes.POINTER(Concat), ci, ci, sz, vp, vp]
    lib.qnn_spatial2d_out_hw.argtypes = [ci, ci, ctypes.POINTER(Spatial2D), ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.qnn_spatial2d_forward.argtypes = [vp, ci, ci, ci, ci, ci, ci, ctypes.POINTER(Spatial2D), vp, vp]
    lib.qnn_depthwise_prepack.argtypes = [ci, ci, fl, vp, ci, ci, ci, ci, vp, ci, ci, ci, ci, ci, vp, ctypes.POINTER(vp)]
    lib.qnn_depthwise_free.argtypes = [vp]
    lib.qnn_depthwise_dequant.argtypes = [vp, vp, vp]
    lib.qnn_depthwise_out_hw.argtypes = [vp, ci, ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.qnn_depthwise_forward.argtypes = [vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(Epilogue), vp, vp]
    lib.qnn_tconv_prepack.argtypes = [ci, ci, fl, vp, ci, ci, ci, ci, vp, ci, ci, ci, vp, ctypes.POINTER(vp)]
    lib.qnn_tconv_free.argtypes = [vp]
    lib.qnn_tconv_dequant.argtypes = [vp, vp, vp]
    lib.qnn_tconv_out_hw.argtypes = [vp, ci, ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.qnn_tconv_forward.argtypes = [vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(Epilogue), vp, vp]
    lib.qnn_gconv_prepack.argtypes = [ci, ci, fl, vp, ci, ci, ci, ci, ci, vp, ci, ci, ci, ci, ci, vp, ctypes.POINTER(vp)]
    lib.qnn_gconv_free.argtypes = [vp]
    lib.qnn_gconv_dequant.argtypes = [vp, vp, vp]
    lib.qnn_gconv_out_hw.argtypes = [vp, ci, ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.qnn_gconv_forward.argtypes = [vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(Epilogue), vp, vp]
    lib.qnn_merge_out_store.argtypes = [ci, ci]
    lib.qnn_merge_forward.argtypes = [ctypes.POINTER(Merge), ci, ci, sz, ci, ci, vp, vp]
    for name in (EXPORTS + EXPORTS_DILATION + EXPORTS_QACT + EXPORTS_MAXACT + EXPORTS_POOL + EXPORTS_SCALED + EXPORTS_CONCAT
                 + EXPORTS_SPATIAL + EXPORTS_DEPTHWISE + EXPORTS_TCONV + EXPORTS_GCONV + EXPORTS_MERGE):   # every symbol the headers declare must be exported
        getattr(lib, name)
    _lib = lib
    return lib


def check(rc, what):
    if rc != QNN_OK:
        msg = load().qnn_last_error().decode(errors="replace")
        if rc == QNN_EUNSUPPORTED and "qnn_quantized_maxact_f32" in msg:     # a refusal with a reason (qnn_abi_maxact.h)
            raise QnnUnsupported("%s: %s" % (what, msg))
        raise QnnError("%s failed (%d): %s" % (what, rc, msg))


IMPL_AUTO, IMPL_VALU, IMPL_MFMA = 0, 1, 2


_conv_impl = IMPL_AUTO


def set_conv_impl(impl):
    """0 auto, 1 VALU kernels only, 2 prefer int8 MFMA (bit-identical results)."""
    global _conv_impl
    check(load().qnn_set_conv_impl(int(impl)), "qnn_set_conv_impl")
    _conv_impl = int(impl)


EPI_NO_STRIP, EPI_NO_STRIP64, EPI_NO_HALO, EPI_NO_LDS16, EPI_NO_FP6 = 1, 2, 4, 8, 16      # qnn_epilogue_t.flags (qnn_abi.h)
EPI_NO_FIRST_TAB, EPI_NO_FIRST_BITS, EPI_NO_HALO_TAB, EPI_NO_FIRST_WIDE, EPI_NO_HALO_EDGE = 32, 64, 128, 256, 512
_default_flags = 0
_default_first = None


def set_option(key, value):
    """TEST / TOOL HELPER of this binding -- the C library keeps no such state (round 4: qnn_set_option is gone from the
    ABI).  Sets what calls made THROUGH THIS MODULE pass per call when the caller says nothing:
      "strip" 0 / 1, "strip64" -1 / 0 / 1, "halo" 0 / 1, "lds16" 0 / 1, "fp6" 0 / 1, "first_tab" 0 / 1, "first_wide" 0 / 1,
      "halo_tab" 0 / 1, "halo_edge" 0 / 1   -> qnn_epilogue_t.flags
                  (QNN_EPI_NO_*): kernel selection only, results bit-identical;
      "first_bits" 0 / 1   -> QNN_EPI_NO_FIRST_BITS in the epilogue that Fold() hands to qnn_fold_prepare: folds of the image
                  entry prepared while it is 0 keep the mode-3 constants in their operand table;
      "first_fixed" / "first_image" 0 / 1   -> a plain float32 input store is declared QNN_STORE_F32_UNIT /
                  QNN_STORE_F32_IMAGE (the typed stores the engines pass explicitly)."""
    global _default_flags, _default_first
    bits = {"strip": EPI_NO_STRIP, "strip64": EPI_NO_STRIP64, "halo": EPI_NO_HALO, "lds16": EPI_NO_LDS16, "fp6": EPI_NO_FP6,
            "first_tab": EPI_NO_FIRST_TAB, "first_wide": EPI_NO_FIRST_WIDE, "first_bits": EPI_NO_FIRST_BITS, "halo_tab": EPI_NO_HALO_TAB,
            "halo_edge": EPI_NO_HALO_EDGE}
    if key in bits:
        _default_flags = (_default_flags | bits[key]) if int(value) == 0 else (_default_flags & ~bits[key])
    elif key in ("first_fixed", "first_image"):
        store = STORE_F32_UNIT if key == "first_fixed" else STORE_F32_IMAGE
        if int(value):
            _default_first = store
        elif _default_first == store:
            _default_first = None
    else:
        raise QnnError("set_option: unknown key %r" % (key,))


def _first_store(x_store):
    return _default_first if (x_store == STORE_F32 and _default_first is not None) else x_store


def conv_impl():
    """The kernel-family preference last set through set_conv_impl()."""
    return _conv_impl


def last_kernel():
    return load().qnn_last_kernel().decode()


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_cuda(t, what):
    """The product path runs on the GPU only; fail loudly otherwise."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a torch.Tensor, got %r" % (what, type(t)))
    if not t.is_cuda:
        raise QnnError("%s: tensor is on %s; the low-bit engine has no CPU path" % (what, t.device))
    if t.dtype != torch.float32:
        raise TypeError("%s: expected float32, got %s" % (what, t.dtype))
    return t.contiguous()


def require_cuda_u8(t, what):
    """Typed image input (QNN_STORE_U8): a uint8 NHWC CUDA tensor, value = code / 255 (utils/load_data.py:40)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a torch.Tensor, got %r" % (what, type(t)))
    if not t.is_cuda:
        raise QnnError("%s: tensor is on %s; the low-bit engine has no CPU path" % (what, t.device))
    if t.dtype != torch.uint8:
        raise TypeError("%s: expected uint8 image bytes, got %s" % (what, t.dtype))
    return t.contiguous()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(None)


def per_word(store):
    """Channels a whole packed word (T2: word pair) covers."""
    return {STORE_BIN: 32, STORE_T2: 32, STORE_I4: 8, STORE_I8: 4}[store]


def words(store, channels):
    if store == STORE_T2:                      # (mask, sign) word pairs per 32 channels
        return 2 * ((channels + 31) // 32)
    pw = per_word(store)
    return (channels + pw - 1) // pw


def store_for_bits(bits):
    """Packed storage able to hold signed `bits`-bit codes (2..8)."""
    if bits <= 4:
        return STORE_I4
    if bits <= 8:
        return STORE_I8
    raise QnnError("no packed storage for %d-bit codes (max 8)" % bits)


# ---------------------------------------------------------------------------
# thin typed wrappers
# ---------------------------------------------------------------------------
def pack(x, channels, fn, nb, store):
    """x: float32 (..., channels) CUDA -> int32 tensor (pixels, words)."""
    x = require_cuda(x, "pack")
    pixels = x.numel() // channels
    out = torch.empty((pixels, words(store, channels)), dtype=torch.int32, device=x.device)
    check(load().qnn_pack_f32(ptr(x), ptr(out), pixels, channels, fn, nb, store, stream_ptr()),
          "qnn_pack_f32")
    return out


def maxact_pack(x, channels, fn, nb, store, workspace, y=None):
    """qnn_maxact_pack_f32 (include/qnn_abi_scaled.h): x float32 (..., channels) CUDA -> int32 (pixels, words) codes of
    quantized_maxrelu / quantized_leakymaxrelu (fn in MAXACT_FNS) at nb bits in STORE_I4 / STORE_I8, scaled by the maximum
    whose bits qnn_maxact_max_f32 left in `workspace` (int32[4] on the device).  y: a float32 tensor shaped like x (x itself
    is allowed) that also receives the values qnn_maxact_apply_f32 would write."""
    x = require_cuda(x, "maxact_pack")
    pixels = x.numel() // channels
    if y is not None and (y.dtype != torch.float32 or not y.is_contiguous() or y.numel() != x.numel() or y.device != x.device):
        raise QnnError("maxact_pack: `y` must be a contiguous float32 tensor of x's size on %s" % (x.device,))
    out = torch.empty((pixels, words(store, channels)), dtype=torch.int32, device=x.device)
    check(load().qnn_maxact_pack_f32(ptr(x), ptr(out), ptr(y), pixels, channels, fn, nb, store, ptr(workspace), stream_ptr()),
          "qnn_maxact_pack_f32")
    return out


def _check_scaled(rc, what):
    """Status of a scaled entry: its own refusals (each names the entry) as QnnUnsupported, the rest through check()."""
    if rc == QNN_EUNSUPPORTED:
        raise QnnUnsupported("%s: %s" % (what, load().qnn_last_error().decode(errors="replace")))
    check(rc, what)


def unpack(p, pixels, channels, store, nb):
    out = torch.empty((pixels, channels), dtype=torch.float32, device=p.device)
    check(load().qnn_unpack_f32(ptr(p), ptr(out), pixels, channels, store, nb, stream_ptr()),
          "qnn_unpack_f32")
    return out


def avgpool_packed(p, store, bits, N, H, W, C, size):
    """AveragePooling2D(size) 'valid' of a packed NHWC tensor -> float32 (N, H//size, W//size, C)."""
    out = torch.empty((N, H // size, W // size, C), dtype=torch.float32, device=p.device)
    check(load().qnn_avgpool_packed_f32(ptr(p), store, bits, N, H, W, C, size, ptr(out), stream_ptr()),
          "qnn_avgpool_packed_f32")
    return out


def _pair(v, what):
    """An int or a pair of ints as Keras takes pool_size / strides: (rows, columns)."""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError("%s must be an integer or a pair of integers, got %r" % (what, v))
        return int(v[0]), int(v[1])
    return int(v), int(v)


def pool2d(x, store, bits, N, H, W, C, mode, size, strides=None, same=False):
    """qnn_pool2d_forward: MaxPooling2D / AveragePooling2D(size, strides, 'same' if same else 'valid') of an NHWC tensor:
    float32 (store = STORE_F32) or int32 packed words (STORE_BIN / _I4 / _I8 at `bits`).  mode: POOL_MAX -> a tensor
    stored like x (packed: (N * Ho * Wo, words) codes at the same bits), POOL_AVG -> float32 (N, Ho, Wo, C).  strides None =
    the window.  Returns (y, Ho, Wo).  The output size comes from the library (qnn_pool2d_out_hw), which refuses a
    'valid' window larger than the image; STORE_T2 raises QnnUnsupported."""
    ph, pw = _pair(size, "size")
    sh, sw = (ph, pw) if strides is None else _pair(strides, "strides")
    desc = Pool2D(int(mode), ph, pw, sh, sw, 1 if same else 0)
    if store == STORE_T2:
        raise QnnUnsupported("pool2d: no pooling on the ternary bit planes (QNN_STORE_T2): unpack, pool, pack")
    Ho, Wo = ctypes.c_int(0), ctypes.c_int(0)
    check(load().qnn_pool2d_out_hw(H, W, ctypes.byref(desc), ctypes.byref(Ho), ctypes.byref(Wo)), "qnn_pool2d_out_hw")
    Ho, Wo = Ho.value, Wo.value
    if store == STORE_F32:
        x = require_cuda(x, "pool2d")
    elif not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.int32 and x.is_contiguous()):
        raise QnnError("pool2d: a packed input must be a contiguous int32 CUDA tensor")
    y_store = store if mode == POOL_MAX else STORE_F32
    if y_store == STORE_F32:
        y = torch.empty((N, Ho, Wo, C), dtype=torch.float32, device=x.device)
    else:
        y = torch.empty((N * Ho * Wo, words(store, C)), dtype=torch.int32, device=x.device)
    check(load().qnn_pool2d_forward(ptr(x), store, bits, N, H, W, C, ctypes.byref(desc), ptr(y), y_store, stream_ptr()),
          "qnn_pool2d_forward")
    return y, Ho, Wo


def pairs2d(v, what):
    """Keras 2.1.3's ZeroPadding2D / Cropping2D argument: an int, a pair of ints (rows, columns: the same on both sides)
    or a pair of pairs ((top, bottom), (left, right)) -> (top, bottom, left, right)."""
    if isinstance(v, numbers.Integral) and not isinstance(v, bool):
        return (int(v),) * 4
    if isinstance(v, (tuple, list)) and len(v) == 2:
        out = []
        for side in v:
            if isinstance(side, numbers.Integral) and not isinstance(side, bool):
                out += [int(side), int(side)]
            elif isinstance(side, (tuple, list)) and len(side) == 2 and \
                    all(isinstance(k, numbers.Integral) and not isinstance(k, bool) for k in side):
                out += [int(side[0]), int(side[1])]
            else:
                out = None
                break
        if out is not None:
            return tuple(out)
    raise ValueError("`%s` should be either an int, a tuple of 2 ints (symmetric_height, symmetric_width), or a tuple of "
                     "2 tuples of 2 ints ((top, bottom), (left, right)). Found: %r" % (what, v))


def spatial_desc(crop=0, up=1, pad=0):
    """qnn_spatial2d_t from Keras' argument forms: crop then repeat then pad."""
    if isinstance(up, (tuple, list)):
        if len(up) != 2:
            raise ValueError("`size` should be an int or a pair of ints, got %r" % (up,))
        uy, ux = int(up[0]), int(up[1])
    else:
        uy = ux = int(up)
    d = Spatial2D()
    d.crop[:] = pairs2d(crop, "cropping")
    d.up[:] = (uy, ux)
    d.pad[:] = pairs2d(pad, "padding")
    return d


def spatial2d_out_hw(H, W, crop=0, up=1, pad=0):
    """qnn_spatial2d_out_hw: (Ho, Wo) of crop -> repeat -> pad on an H x W image; touches no device."""
    desc = spatial_desc(crop, up, pad)
    Ho, Wo = ctypes.c_int(0), ctypes.c_int(0)
    check(load().qnn_spatial2d_out_hw(int(H), int(W), ctypes.byref(desc), ctypes.byref(Ho), ctypes.byref(Wo)),
          "qnn_spatial2d_out_hw")
    return Ho.value, Wo.value


def spatial2d(x, store, bits, N, H, W, C, crop=0, up=1, pad=0):
    """qnn_spatial2d_forward: Cropping2D(crop), then UpSampling2D(up) (nearest), then ZeroPadding2D(pad) of an NHWC tensor:
    float32 (store = STORE_F32) -> float32 (N, Ho, Wo, C), or int32 packed words (STORE_BIN / _I4 / _I8 at `bits`,
    STORE_T2) as pack() writes them -> (N * Ho * Wo, words) codes of the same store and bits, spare bits zero.  Codes are
    copied, never re-quantised.  Returns (y, Ho, Wo).  A pad on STORE_BIN raises QnnUnsupported (a +-1 code has no zero)."""
    desc = spatial_desc(crop, up, pad)
    Ho, Wo = ctypes.c_int(0), ctypes.c_int(0)
    check(load().qnn_spatial2d_out_hw(int(H), int(W), ctypes.byref(desc), ctypes.byref(Ho), ctypes.byref(Wo)),
          "qnn_spatial2d_out_hw")
    Ho, Wo = Ho.value, Wo.value
    if store == STORE_F32:
        x = require_cuda(x, "spatial2d")
        n = N * H * W * C
    else:
        if store not in (STORE_BIN, STORE_T2, STORE_I4, STORE_I8):
            raise QnnError("spatial2d: store=%r (float32 or a packed activation store)" % (store,))
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.int32 and x.is_contiguous()):
            raise QnnError("spatial2d: a packed input must be a contiguous int32 CUDA tensor")
        n = N * H * W * words(store, C)
    if x.numel() != n:
        raise QnnError("spatial2d: the input holds %d elements, %d x %d x %d pixels of %d channels are %d"
                       % (x.numel(), N, H, W, C, n))
    if store == STORE_F32:
        y = torch.empty((N, Ho, Wo, C), dtype=torch.float32, device=x.device)
    else:
        y = torch.empty((N * Ho * Wo, words(store, C)), dtype=torch.int32, device=x.device)
    rc = load().qnn_spatial2d_forward(ptr(x), int(store), int(bits), int(N), int(H), int(W), int(C), ctypes.byref(desc),
                                      ptr(y), stream_ptr())
    if rc == QNN_EUNSUPPORTED:
        raise QnnUnsupported("qnn_spatial2d_forward: " + load().qnn_last_error().decode(errors="replace"))
    check(rc, "qnn_spatial2d_forward")
    return y, Ho, Wo


def concat(tensors, channels, store, bits, pixels):
    """qnn_concat_forward: Concatenate(axis=-1) of 1 .. CONCAT_MAX tensors that share `pixels` pixels: float32 (store =
    STORE_F32; tensor i holds pixels * channels[i] values) -> float32 (pixels, sum of the channels), or int32 packed words
    (STORE_BIN / _I4 / _I8 at `bits`, STORE_T2) as pack() writes them -> the packed words of the concatenation, spare bits
    zero.  Codes are copied, never re-quantised.  CUDA tensors only: there is no CPU path."""
    tensors, channels = list(tensors), [int(c) for c in channels]
    if len(tensors) != len(channels):
        raise ValueError("concat: %d tensors but %d channel counts" % (len(tensors), len(channels)))
    if not 1 <= len(tensors) <= CONCAT_MAX:
        raise QnnError("concat: %d inputs (qnn_concat_forward takes 1 .. %d)" % (len(tensors), CONCAT_MAX))
    if store not in (STORE_F32, STORE_BIN, STORE_T2, STORE_I4, STORE_I8):
        raise QnnError("concat: store=%r (float32 or a packed activation store)" % (store,))
    if min(channels) < 1:
        raise QnnError("concat: channels=%r (every input has at least one)" % (channels,))
    pixels = int(pixels)
    dt = torch.float32 if store == STORE_F32 else torch.int32
    xs = []
    for i, (t, c) in enumerate(zip(tensors, channels)):
        if store == STORE_F32:
            t = require_cuda(t, "concat")
            n = pixels * c
        else:
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
                raise QnnError("concat: a packed input must be a contiguous int32 CUDA tensor")
            n = pixels * words(store, c)
        if t.numel() != n:
            raise QnnError("concat: input %d holds %d elements, %d pixels of %d channels are %d" % (i, t.numel(), pixels, c, n))
        xs.append(t)
    desc = Concat()
    desc.n = len(xs)
    for i, (t, c) in enumerate(zip(xs, channels)):
        desc.channels[i] = c
        desc.x[i] = t.data_ptr()
    total = sum(channels)
    cols = total if store == STORE_F32 else words(store, total)
    y = torch.empty((pixels, cols), dtype=dt, device=xs[0].device)
    rc = load().qnn_concat_forward(ctypes.byref(desc), int(store), int(bits), pixels, ptr(y), stream_ptr())
    if rc == QNN_EUNSUPPORTED:
        raise QnnUnsupported("qnn_concat_forward: " + load().qnn_last_error().decode(errors="replace"))
    check(rc, "qnn_concat_forward")
    return y


def merge_out_store(op, store):
    """qnn_merge_out_store: the store the merge `op` ("add" | "sub" | "mul" | "avg" | "max" | "min", or a MERGE_* number)
    of inputs of `store` is written in: `store` itself where the result is again a code, else STORE_F32."""
    if isinstance(op, str) and op not in MERGE_OPS:
        raise QnnError("merge: fn=%r (one of %s)" % (op, ", ".join(MERGE_OPS)))
    rc = load().qnn_merge_out_store(MERGE_OPS[op] if isinstance(op, str) else int(op), int(store))
    if rc < 0:
        check(rc, "qnn_merge_out_store")
    return rc


def merge(xs, op, store, bits, pixels, channels):
    """qnn_merge_forward: the element-wise merge `op` ("add" | "sub" | "mul" | "avg" | "max" | "min", or a MERGE_* number)
    of 2 .. MERGE_MAX tensors of one shape, `pixels` rows of `channels` values: float32 (store = STORE_F32), or int32 packed
    words (STORE_BIN / _I4 / _I8 at `bits`, STORE_T2) as pack() writes them.  Returns (tensor, out_store): the packed words
    of the result where it is again a code (max / min; mul of BIN and T2), spare bits zero, else float32 (pixels, channels).
    CUDA tensors only: there is no CPU path."""
    xs = list(xs)
    out_store = merge_out_store(op, store)
    opn = MERGE_OPS[op] if isinstance(op, str) else int(op)
    if not 2 <= len(xs) <= MERGE_MAX:
        raise QnnError("merge: %d inputs (qnn_merge_forward takes 2 .. %d)" % (len(xs), MERGE_MAX))
    if opn == MERGE_SUB and len(xs) != 2:
        raise QnnError("merge: a subtraction takes exactly 2 inputs, got %d" % len(xs))
    pixels, channels = int(pixels), int(channels)
    if channels < 1:
        raise QnnError("merge: channels=%d" % channels)
    cols = channels if store == STORE_F32 else words(store, channels)
    ts = []
    for i, t in enumerate(xs):
        if store == STORE_F32:
            t = require_cuda(t, "merge")
        elif not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
            raise QnnError("merge: a packed input must be a contiguous int32 CUDA tensor")
        if t.numel() != pixels * cols:
            raise QnnError("merge: input %d holds %d elements, %d pixels of %d channels are %d"
                           % (i, t.numel(), pixels, channels, pixels * cols))
        ts.append(t)
    desc = Merge()
    desc.n, desc.op = len(ts), opn
    for i, t in enumerate(ts):
        desc.x[i] = t.data_ptr()
    if out_store == STORE_F32:
        y = torch.empty((pixels, channels), dtype=torch.float32, device=ts[0].device)
    else:
        y = torch.empty((pixels, cols), dtype=torch.int32, device=ts[0].device)
    rc = load().qnn_merge_forward(ctypes.byref(desc), int(store), int(bits), pixels, channels, out_store, ptr(y), stream_ptr())
    if rc == QNN_EUNSUPPORTED:
        raise QnnUnsupported("qnn_merge_forward: " + load().qnn_last_error().decode(errors="replace"))
    check(rc, "qnn_merge_forward")
    return y, out_store


def softmax(x, out=None):
    """qnn_softmax_f32 over the last axis (float64 inside, one rounding): Dense(..., activation='softmax')."""
    x = require_cuda(x, "softmax input").contiguous()
    assert x.dtype == torch.float32
    y = out if out is not None else torch.empty_like(x)
    cols = x.shape[-1]
    check(load().qnn_softmax_f32(ptr(x), ptr(y), x.numel() // cols, cols, stream_ptr()), "qnn_softmax_f32")
    return y


def avgpool_dense_softmax(weights, packed, store, bits, N, H, W, C, size, softmax=True, bn_inv=None, bn_shift=None,
                          logits=None, out=None, fn=FN_NONE):
    """qnn_avgpool_dense_softmax_forward: AveragePooling2D(size) -> Flatten -> Dense [-> softmax] of a packed NHWC tensor
    in one launch (models/resnet.py:134-140), bit-identical to avgpool_packed -> dense (QNN_STORE_F32 handle) -> softmax.
    Returns the (N, classes) float32 tensor (the logits with softmax=False); `logits`: an (N, classes) float32 tensor
    that also receives the logits.  Raises QnnUnsupported where the library has no fused kernel: issue the three calls."""
    classes = weights.shape[3]
    y = out if out is not None else torch.empty((N, classes), dtype=torch.float32, device=packed.device)
    for t, what in ((y, "out"), (logits, "logits")):
        if t is not None and (tuple(t.shape) != (N, classes) or t.dtype != torch.float32 or not t.is_contiguous()
                              or t.device != packed.device):
            raise QnnError("avgpool_dense_softmax: `%s` must be a contiguous float32 tensor of shape %s on %s"
                           % (what, (N, classes), packed.device))
    epi = make_epilogue(bn_inv, bn_shift, fn, 0, 1, STORE_F32)
    rc = load().qnn_avgpool_dense_softmax_forward(weights.handle, ptr(packed), store, bits, N, H, W, C, size,
                                                  ctypes.byref(epi), 1 if softmax else 0, ptr(logits), ptr(y), stream_ptr())
    if rc == QNN_EUNSUPPORTED:
        raise QnnUnsupported("qnn_avgpool_dense_softmax_forward: " + load().qnn_last_error().decode(errors="replace"))
    check(rc, "qnn_avgpool_dense_softmax_forward")
    return y


# Handles released while a HIP stream capture is in progress (Python's cycle collector can run a __del__ anywhere, e.g.
# inside `with torch.cuda.graph(g)`): hipFree is not permitted during a capture and would invalidate it, so the handle is
# parked here and freed at the next safe point (the next handle creation, or release_deferred()).
_deferred = []


def _release(fn_name, handle):
    if not (handle and handle.value) or _lib is None:
        return
    try:
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
    except Exception:
        capturing = False
    if capturing:
        _deferred.append((fn_name, handle.value))
    else:
        getattr(_lib, fn_name)(handle)


def release_deferred():
    """Free the handles whose owners died during a stream capture (no-op while a capture is in progress)."""
    if not _deferred or _lib is None:
        return
    try:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            return
    except Exception:
        return
    while _deferred:
        fn_name, value = _deferred.pop()
        getattr(_lib, fn_name)(ctypes.c_void_p(value))


class Weights:
    """Owner of an opaque qnn_weights_t handle."""

    def __init__(self, wkind, wbits, H, kernel, bias, stride, same_pad, store, dilation=(1, 1)):
        """dilation: the layer's dilation_rate as (rows, columns); anything but (1, 1) goes through
        qnn_prepack_weights_dilated, which refuses it together with stride != 1."""
        kernel = require_cuda(kernel, "prepack kernel")
        if kernel.dim() == 2:
            kh = kw = 1
            cin, cout = kernel.shape
        else:
            kh, kw, cin, cout = kernel.shape
        bias = require_cuda(bias, "prepack bias") if bias is not None else None
        self.shape = (kh, kw, cin, cout)
        self.wkind = wkind
        self.store = store
        self.stride = stride
        self.same_pad = same_pad
        self.dilation = (int(dilation[0]), int(dilation[1]))
        self.handle = ctypes.c_void_p(None)
        release_deferred()
        if self.dilation == (1, 1):
            check(load().qnn_prepack_weights(wkind, wbits, float(H), ptr(kernel), kh, kw, cin, cout,
                                             ptr(bias), stride, 1 if same_pad else 0, store,
                                             stream_ptr(), ctypes.byref(self.handle)),
                  "qnn_prepack_weights")
        else:
            check(load().qnn_prepack_weights_dilated(wkind, wbits, float(H), ptr(kernel), kh, kw, cin, cout,
                                                     ptr(bias), stride, 1 if same_pad else 0, self.dilation[0],
                                                     self.dilation[1], store, stream_ptr(), ctypes.byref(self.handle)),
                  "qnn_prepack_weights_dilated")
        self.device = kernel.device

    def check(self):
        """qnn_weights_check: synchronise the current stream and raise QnnError if a restricted-domain kernel of this
        layer (the opt-in fixed-point first layer: inputs in [0, 1]) met a value outside its domain since the last check."""
        check(load().qnn_weights_check(self.handle, stream_ptr()), "qnn_weights_check")

    def dequant(self):
        kh, kw, cin, cout = self.shape
        out = torch.empty((kh, kw, cin, cout), dtype=torch.float32, device=self.device)
        check(load().qnn_weights_dequant(self.handle, ptr(out), stream_ptr()), "qnn_weights_dequant")
        return out

    def __del__(self):
        try:
            _release("qnn_free_weights", self.handle)
            self.handle = ctypes.c_void_p(None)
        except Exception:
            pass


def out_hw(size, k, stride, same_pad, dilation=1):
    """Output size of one axis, the rule of csrc/qnn_conv_geom.h on the effective window dilation * (k - 1) + 1: 'valid'
    with a window larger than the image is 0."""
    if same_pad:
        return -(-size // stride)
    ke = dilation * (k - 1) + 1
    return (size - ke) // stride + 1 if size >= ke else 0


def _stored_hw(what, w, H, W, pool):
    """(Hp, Wp) of a conv call's stored output; an empty one (before or after pooling) is refused here, before any
    library call, as conv_describe refuses it ("empty output")."""
    kh, kw = w.shape[0], w.shape[1]
    dh, dw = getattr(w, "dilation", (1, 1))
    Ho, Wo = out_hw(H, kh, w.stride, w.same_pad, dh), out_hw(W, kw, w.stride, w.same_pad, dw)
    if Ho // pool <= 0 or Wo // pool <= 0:
        raise QnnError("%s: empty output: %dx%d input, %dx%d window%s, stride %d, %s padding gives %dx%d%s"
                       % (what, H, W, kh, kw, " dilated %dx%d" % (dh, dw) if (dh, dw) != (1, 1) else "", w.stride,
                          "same" if w.same_pad else "valid", Ho, Wo, ", pooled by %d" % pool if pool != 1 else ""))
    return Ho // pool, Wo // pool


def make_epilogue(bn_inv, bn_shift, fn, act_bits, pool, out_store, res=None, res_store=STORE_F32,
                  res_bits=0, post_scale=1.0, trick=None, fold=None, domain_flag=None, flags=None, proj=None):
    """trick: None (the reference's lr-multiplier identity trick is the identity) or the (c, s) float32 pair of its
    OUTPUT side, `faithful_trick(klm, promotion)`.  fold: a Fold prepared for exactly this layer and epilogue.
    proj: (weights of the 1x1 strides-2 projection, packed block input, H, W, x_bits) -- the shortcut computed inside the
    launch (qnn_projection_t); the returned epilogue keeps the descriptor alive as `_proj`."""
    tc, ts = (float(trick[0]), float(trick[1])) if trick is not None else (0.0, 0.0)
    pj = None
    if proj is not None:
        pw, px, pH, pW, pbits = proj
        pj = Projection(pw.handle.value, ptr(px).value, int(pH), int(pW), int(pbits))
    e = Epilogue(ptr(bn_inv).value, ptr(bn_shift).value, fn, act_bits, pool, out_store,
                 ptr(res).value, res_store, res_bits, float(post_scale), tc, ts,
                 fold.handle.value if fold is not None else None,
                 _default_flags if flags is None else int(flags),
                 ptr(domain_flag).value if domain_flag is not None else None,
                 ctypes.addressof(pj) if pj is not None else None)
    e._proj = pj
    return e


class Fold:
    """Owner of a qnn_fold_t: the epilogue of one layer (bias, BN, [shortcut merge], quantized_tanh) folded to a slope and
    an accumulator offset per channel and PROVEN equal to the float32 chain on every point of the layer's accumulator
    domain (qnn_fold_prepare, include/qnn_abi.h).  `usable` False = some channel has no exact fold: the kernels keep the
    chain (bit-identical results either way).  Returns None from `try_prepare` where the library folds nothing
    (other bit widths, float32 shortcut, ...)."""

    def __init__(self, w, x_store, x_bits, bn_inv, bn_shift, fn, act_bits, out_store, res=None, res_store=STORE_F32,
                 res_bits=0, post_scale=1.0):
        self._keep = (w, bn_inv, bn_shift)
        self.handle = ctypes.c_void_p(None)
        release_deferred()
        epi = make_epilogue(bn_inv, bn_shift, fn, act_bits, 1, out_store, res, res_store, res_bits, post_scale)
        rc = load().qnn_fold_prepare(w.handle, x_store, x_bits, ctypes.byref(epi), stream_ptr(), ctypes.byref(self.handle))
        self.rc = rc
        if rc != QNN_OK:
            self.handle = ctypes.c_void_p(None)
            if rc == QNN_EUNSUPPORTED and (w.dilation != (1, 1) or fn in MAXACT_FNS):   # not a shape the library may fold one day: a refusal
                raise QnnUnsupported("qnn_fold_prepare: " + load().qnn_last_error().decode(errors="replace"))
            if rc != QNN_EUNSUPPORTED:
                check(rc, "qnn_fold_prepare")
            return
        info = FoldInfo()
        check(load().qnn_fold_info(self.handle, ctypes.byref(info)), "qnn_fold_info")
        self.channels, self.folded, self.usable = info.channels, info.folded, bool(info.usable)
        self.points, self.acc_lo, self.acc_hi = info.points, info.acc_lo, info.acc_hi
        self.shortcut_codes, self.mode = info.shortcut_codes, info.mode

    @classmethod
    def try_prepare(cls, *a, **kw):
        f = cls(*a, **kw)
        return f if f.handle.value else None

    def constants(self, device):
        A = torch.empty(self.channels, dtype=torch.float32, device=device)
        b = torch.empty(self.channels, dtype=torch.int32, device=device)
        check(load().qnn_fold_constants(self.handle, ptr(A), ptr(b), None, stream_ptr()), "qnn_fold_constants")
        return A, b

    def eval(self, c, acc, sc=None):
        """The folded epilogue of channel c on int32 CUDA tensors acc (true accumulator units) [and sc]: int32 codes."""
        out = torch.empty_like(acc)
        check(load().qnn_fold_eval(self.handle, int(c), ptr(acc), ptr(sc), ptr(out), acc.numel(), stream_ptr()),
              "qnn_fold_eval")
        return out

    def __del__(self):
        try:
            _release("qnn_fold_free", self.handle)
            self.handle = ctypes.c_void_p(None)
        except Exception:
            pass


def faithful_trick(klm, promotion="nep50"):
    """The two float32 constants of `(o - (1. - 1./klm) * o) * klm` (binary_layers.py:175-176) as the reference forms
    them: `promotion` = "nep50" (numpy >= 2: everything stays float32) or "legacy" (numpy < 2: `1. - 1./np.float32`
    is float64, cast to float32 when it meets the tensor)."""
    import numpy as np
    k = np.float32(klm)
    if promotion == "legacy":
        c = np.float32(1.0 - 1.0 / float(k))
    elif promotion == "nep50":
        c = np.float32(1.0) - np.float32(1.0) / k
    else:
        raise ValueError(promotion)
    return float(np.float32(c)), float(k)


def conv2d(w, x, x_store, x_bits, N, H, W, bn_inv=None, bn_shift=None, fn=FN_NONE, act_bits=0,
           pool=1, out_store=STORE_F32, res=None, res_store=STORE_F32, res_bits=0, post_scale=1.0, out=None, trick=None,
           fold=None, domain_flag=None, proj=None, x_scale=None):
    """Run qnn_conv2d_forward; x is a float32 NHWC tensor, a uint8 NHWC tensor or an int32 packed tensor.
    Returns (y, Hp, Wp): y float32 (N,Hp,Wp,cout) or int32 (N*Hp*Wp, words); `out` = a tensor of that shape to write
    into instead of a fresh one.  proj: see make_epilogue (raises QnnUnsupported where no kernel computes it).
    x_scale: the workspace word of maxact_pack whose codes x holds -> qnn_conv2d_forward_scaled (qnn_abi_scaled.h)."""
    cout = w.shape[3]
    Ho, Wo = _stored_hw("conv2d", w, H, W, pool)
    if out_store == STORE_F32:
        shape, dt = (N, Ho, Wo, cout), torch.float32
    else:
        shape, dt = (N * Ho * Wo, words(out_store, cout)), torch.int32
    if out is None:
        y = torch.empty(shape, dtype=dt, device=x.device)
    else:
        if tuple(out.shape) != shape or out.dtype != dt or not out.is_contiguous() or out.device != x.device:
            raise QnnError("conv2d: `out` must be a contiguous %s tensor of shape %s on %s" % (dt, shape, x.device))
        y = out
    epi = make_epilogue(bn_inv, bn_shift, fn, act_bits, pool, out_store, res, res_store, res_bits, post_scale, trick, fold,
                        domain_flag, proj=proj)
    if x_scale is not None:
        _check_scaled(load().qnn_conv2d_forward_scaled(w.handle, ptr(x), x_store, x_bits, N, H, W, ctypes.byref(epi),
                                                       ptr(x_scale), ptr(y), stream_ptr()), "qnn_conv2d_forward_scaled")
        return y, Ho, Wo
    rc = load().qnn_conv2d_forward(w.handle, ptr(x), _first_store(x_store), x_bits, N, H, W, ctypes.byref(epi),
                                   ptr(y), stream_ptr())
    if proj is not None and rc == QNN_EUNSUPPORTED:
        raise QnnUnsupported("qnn_conv2d_forward: " + load().qnn_last_error().decode(errors="replace"))
    check(rc, "qnn_conv2d_forward")
    return y, Ho, Wo



def conv2d_dense(wc, wd, x, x_store, x_bits, N, H, W, c_inv, c_shift, c_fn, c_act_bits, d_inv, d_shift, out=None, fold=None):
    """qnn_conv2d_dense_forward: the last conv group (2x2 pool, packed int4 codes) and the dense head behind it in one
    launch.  Returns the (N, units) float32 logits, or None when no fused kernel covers the pair (QNN_EUNSUPPORTED)."""
    units = wd.shape[3]
    _stored_hw("conv2d_dense", wc, H, W, 2)
    y = out if out is not None else torch.empty((N, units), dtype=torch.float32, device=x.device)
    ec = make_epilogue(c_inv, c_shift, c_fn, c_act_bits, 2, STORE_I4, fold=fold)
    ed = make_epilogue(d_inv, d_shift, FN_NONE, 0, 1, STORE_F32)
    rc = load().qnn_conv2d_dense_forward(wc.handle, wd.handle, ptr(x), x_store, x_bits, N, H, W, ctypes.byref(ec),
                                         ctypes.byref(ed), ptr(y), stream_ptr())
    if rc == QNN_EUNSUPPORTED:
        if wc.dilation != (1, 1):                 # refused for its dilation, not for a shape: say so
            raise QnnUnsupported("qnn_conv2d_dense_forward: " + load().qnn_last_error().decode(errors="replace"))
        return None
    check(rc, "qnn_conv2d_dense_forward")
    return y


class BoundHead:
    """qnn_conv2d_dense_forward with everything bound once (see BoundStep)."""

    def __init__(self, wc, wd, x_store, x_bits, N, H, W, c_inv, c_shift, c_fn, c_act_bits, d_inv, d_shift, x, fold=None):
        self._keep = (wc, wd, c_inv, c_shift, d_inv, d_shift, x, fold)
        self._ec = make_epilogue(c_inv, c_shift, c_fn, c_act_bits, 2, STORE_I4, fold=fold)
        self._ed = make_epilogue(d_inv, d_shift, FN_NONE, 0, 1, STORE_F32)
        self._x = x.data_ptr()
        self._fn = load().qnn_conv2d_dense_forward
        self._a = (wc.handle, wd.handle)
        self._mid = (x_store, x_bits, N, H, W, ctypes.byref(self._ec), ctypes.byref(self._ed))

    def __call__(self, stream, x_ptr=None, y_ptr=None):
        rc = self._fn(self._a[0], self._a[1], ctypes.c_void_p(x_ptr or self._x), *self._mid, ctypes.c_void_p(y_ptr),
                      ctypes.c_void_p(stream))
        if rc != QNN_OK:
            check(rc, "qnn_conv2d_dense_forward")


class BoundStep:
    """qnn_conv2d_forward / qnn_dense_forward with everything bound once: a launch is then one foreign call, not a page
    of Python.  `x` / `y` are the step's static input / output tensors; either pointer can be overridden per call (a
    pipeline's first step reads the caller's batch in place, its last step writes into the caller's result)."""

    def __init__(self, kind, w, x_store, x_bits, N, H, W, bn_inv, bn_shift, fn, act_bits, pool, out_store, x, y,
                 trick=None, fold=None):
        self._keep = (w, bn_inv, bn_shift, x, y, fold)
        self._epi = make_epilogue(bn_inv, bn_shift, fn, act_bits, pool, out_store, trick=trick, fold=fold)
        self._x = x.data_ptr() if x is not None else 0
        self._y = y.data_ptr() if y is not None else 0
        lib = load()
        if kind == "conv":
            self._fn = lib.qnn_conv2d_forward
            self._mid = (_first_store(x_store), x_bits, N, H, W, ctypes.byref(self._epi))
        else:
            self._fn = lib.qnn_dense_forward
            self._mid = (x_store, x_bits, N, ctypes.byref(self._epi))
        self._h = w.handle
        self._what = "qnn_%s_forward" % ("conv2d" if kind == "conv" else "dense")

    def __call__(self, stream, x_ptr=None, y_ptr=None, flag_ptr=None):
        if flag_ptr is not None:
            self._epi.domain_flag = flag_ptr       # the caller's domain-flag word of THIS batch (engine "auto" mode)
        rc = self._fn(self._h, ctypes.c_void_p(x_ptr or self._x), *self._mid, ctypes.c_void_p(y_ptr or self._y),
                      ctypes.c_void_p(stream))
        if rc != QNN_OK:
            check(rc, self._what)


def conv2d_f32in(w, x, in_fn, in_bits, bn_inv=None, bn_shift=None, fn=FN_NONE, act_bits=0, pool=1,
                 out_store=STORE_F32):
    """qnn_conv2d_forward_f32in: float32 NHWC x, activation clip `in_fn` fused on load."""
    x = require_cuda(x, "conv2d_f32in")
    N, H, W, _ = x.shape
    cout = w.shape[3]
    Ho, Wo = _stored_hw("conv2d_f32in", w, H, W, pool)
    if out_store == STORE_F32:
        y = torch.empty((N, Ho, Wo, cout), dtype=torch.float32, device=x.device)
    else:
        y = torch.empty((N * Ho * Wo, words(out_store, cout)), dtype=torch.int32, device=x.device)
    need = load().qnn_conv2d_workspace_bytes(w.handle, N, H, W)
    ws = torch.empty((max(need, 4) + 3) // 4, dtype=torch.int32, device=x.device)
    epi = make_epilogue(bn_inv, bn_shift, fn, act_bits, pool, out_store)
    check(load().qnn_conv2d_forward_f32in(w.handle, ptr(x), in_fn, in_bits, N, H, W, ctypes.byref(epi),
                                          ptr(y), ptr(ws), ws.numel() * 4, stream_ptr()),
          "qnn_conv2d_forward_f32in")
    return y, Ho, Wo


def dense(w, x, x_store, x_bits, N, bn_inv=None, bn_shift=None, fn=FN_NONE, act_bits=0,
          out_store=STORE_F32, out=None, x_scale=None):
    """Run qnn_dense_forward; x_scale: as in conv2d -> qnn_dense_forward_scaled."""
    cout = w.shape[3]
    if out_store == STORE_F32:
        shape, dt = (N, cout), torch.float32
    else:
        shape, dt = (N, words(out_store, cout)), torch.int32
    if out is None:
        y = torch.empty(shape, dtype=dt, device=x.device)
    else:
        if tuple(out.shape) != shape or out.dtype != dt or not out.is_contiguous() or out.device != x.device:
            raise QnnError("dense: `out` must be a contiguous %s tensor of shape %s on %s" % (dt, shape, x.device))
        y = out
    epi = make_epilogue(bn_inv, bn_shift, fn, act_bits, 1, out_store)
    if x_scale is not None:
        _check_scaled(load().qnn_dense_forward_scaled(w.handle, ptr(x), x_store, x_bits, N, ctypes.byref(epi), ptr(x_scale),
                                                      ptr(y), stream_ptr()), "qnn_dense_forward_scaled")
        return y
    check(load().qnn_dense_forward(w.handle, ptr(x), x_store, x_bits, N, ctypes.byref(epi), ptr(y),
                                   stream_ptr()), "qnn_dense_forward")
    return y


class _SideWeights:
    """What DepthwiseWeights, TConvWeights and GConvWeights share: the owner of a handle behind the C symbols
    <_prefix>_prepack / _dequant / _out_hw / _free.  A subclass checks its kernel layout and bias size and hands _prepack
    the arguments its entry takes between the kernel pointer and the stream."""
    _prefix = _what = None

    def _tensors(self, layout, kernel, bias):
        kernel = require_cuda(kernel, self._what + " prepack kernel")
        if kernel.dim() != 4:
            raise QnnError("%s prepack: the kernel must be %s, got %s" % (self._what, layout, tuple(kernel.shape)))
        return kernel, (require_cuda(bias, self._what + " prepack bias") if bias is not None else None)

    def _prepack(self, wkind, wbits, H, kernel, stride, same_pad, store, *args):
        self.shape = tuple(kernel.shape)
        self.wkind, self.wbits, self.store = wkind, wbits, store
        self.stride, self.same_pad = int(stride), bool(same_pad)
        self.handle = ctypes.c_void_p(None)
        release_deferred()
        name = self._prefix + "_prepack"
        rc = getattr(load(), name)(wkind, wbits, float(H), ptr(kernel), *args, stream_ptr(), ctypes.byref(self.handle))
        if rc == QNN_EUNSUPPORTED:
            raise QnnUnsupported(name + ": " + load().qnn_last_error().decode(errors="replace"))
        check(rc, name)
        self.device = kernel.device

    def dequant(self):
        out = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        check(getattr(load(), self._prefix + "_dequant")(self.handle, ptr(out), stream_ptr()), self._prefix + "_dequant")
        return out

    def out_hw(self, H, W):
        Ho, Wo = ctypes.c_int(0), ctypes.c_int(0)
        check(getattr(load(), self._prefix + "_out_hw")(self.handle, int(H), int(W), ctypes.byref(Ho), ctypes.byref(Wo)),
              self._prefix + "_out_hw")
        return Ho.value, Wo.value

    def __del__(self):
        try:
            _release(self._prefix + "_free", self.handle)
            self.handle = ctypes.c_void_p(None)
        except Exception:
            pass


def _side_forward(prefix, what, w, x, x_store, x_bits, N, H, W, Ho, Wo, bn_inv, bn_shift, fn, act_bits, out_store, out,
                  epilogue):
    """The body depthwise(), tconv() and gconv() share, from the input check to <prefix>_forward."""
    if x_store == STORE_F32:
        x = require_cuda(x, what)
    elif not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.int32 and x.is_contiguous()):
        raise QnnError("%s: a packed input must be a contiguous int32 CUDA tensor" % what)
    if out_store == STORE_F32:
        shape, dt = (N, Ho, Wo, w.cout), torch.float32
    else:
        shape, dt = (N * Ho * Wo, words(out_store, w.cout)), torch.int32
    if out is None:
        y = torch.empty(shape, dtype=dt, device=x.device)
    else:
        if tuple(out.shape) != shape or out.dtype != dt or not out.is_contiguous() or out.device != x.device:
            raise QnnError("%s: `out` must be a contiguous %s tensor of shape %s on %s" % (what, dt, shape, x.device))
        y = out
    epi = epilogue if epilogue is not None else make_epilogue(bn_inv, bn_shift, fn, act_bits, 1, out_store, flags=0)
    name = prefix + "_forward"
    rc = getattr(load(), name)(w.handle, ptr(x), int(x_store), int(x_bits), int(N), int(H), int(W), ctypes.byref(epi), ptr(y),
                               stream_ptr())
    if rc == QNN_EUNSUPPORTED:
        raise QnnUnsupported(name + ": " + load().qnn_last_error().decode(errors="replace"))
    check(rc, name)
    return y, Ho, Wo


def _refuse_empty(what, w, H, W, Ho, Wo):
    if Ho <= 0 or Wo <= 0:
        raise QnnError("%s: empty output: %dx%d input, %dx%d window dilated %dx%d, stride %d, %s padding"
                       % (what, H, W, w.shape[0], w.shape[1], w.dilation[0], w.dilation[1], w.stride,
                          "same" if w.same_pad else "valid"))


class DepthwiseWeights(_SideWeights):
    """Owner of an opaque qnn_dw_weights_t handle (include/qnn_abi_depthwise.h).  kernel: float32 CUDA tensor in Keras'
    depthwise layout (kh, kw, C, depth_multiplier); bias: (C * depth_multiplier,) or None."""
    _prefix, _what = "qnn_depthwise", "depthwise"

    def __init__(self, wkind, wbits, H, kernel, bias, stride, same_pad, store, dilation=(1, 1)):
        kernel, bias = self._tensors("(kh, kw, C, depth_multiplier)", kernel, bias)
        kh, kw, C, M = kernel.shape
        if bias is not None and bias.numel() != C * M:
            raise QnnError("depthwise prepack: bias of %d values for %d x %d channels" % (bias.numel(), C, M))
        self.cout = C * M
        self.dilation = (int(dilation[0]), int(dilation[1]))
        self._prepack(wkind, wbits, H, kernel, stride, same_pad, store, kh, kw, C, M, ptr(bias), int(stride),
                      1 if same_pad else 0, self.dilation[0], self.dilation[1], store)


def depthwise(w, x, x_store, x_bits, N, H, W, bn_inv=None, bn_shift=None, fn=FN_NONE, act_bits=0, out_store=STORE_F32,
              out=None, epilogue=None):
    """qnn_depthwise_forward: x is a float32 NHWC CUDA tensor (x_store = STORE_F32) or int32 packed words as pack()
    writes them.  Returns (y, Ho, Wo): y float32 (N, Ho, Wo, C * M) or int32 (N * Ho * Wo, words).  `epilogue`: a ready
    Epilogue instead of the keyword fields (tests of the refusals).  A refusal with QNN_EUNSUPPORTED raises QnnUnsupported."""
    Ho, Wo = w.out_hw(H, W)
    _refuse_empty("depthwise", w, H, W, Ho, Wo)
    return _side_forward("qnn_depthwise", "depthwise", w, x, x_store, x_bits, N, H, W, Ho, Wo, bn_inv, bn_shift, fn, act_bits,
                         out_store, out, epilogue)


def tconv_out_hw(size, k, stride, same_pad):
    """Output size of one axis of a transposed convolution (csrc/qnn_conv_geom.h, qnn_tconv_out_pad)."""
    return size * stride + (0 if same_pad else max(k - stride, 0))


def tconv_takes_mfma(kh, kw, stride, store, cout, cin, out_store):
    """The shape half of the route rule of the matrix-pipe form (include/qnn_abi_tconv.h); the library adds 16-byte
    aligned pointers and an input image below 2^31 bytes."""
    return (stride == 2 and kh == kw and 2 <= kh <= 4 and store in (STORE_I4, STORE_I8) and out_store == store and
            cin % 64 == 0 and cin <= 16384 and cout % 16 == 0)


class TConvWeights(_SideWeights):
    """Owner of an opaque qnn_tconv_weights_t handle (include/qnn_abi_tconv.h).  kernel: float32 CUDA tensor in Keras'
    Conv2DTranspose layout (kh, kw, Cout, Cin); bias: (Cout,) or None."""
    _prefix, _what = "qnn_tconv", "tconv"

    def __init__(self, wkind, wbits, H, kernel, bias, stride, same_pad, store):
        kernel, bias = self._tensors("(kh, kw, Cout, Cin)", kernel, bias)
        kh, kw, cout, cin = kernel.shape
        if bias is not None and bias.numel() != cout:
            raise QnnError("tconv prepack: bias of %d values for %d filters" % (bias.numel(), cout))
        self.cout, self.cin = cout, cin
        self._prepack(wkind, wbits, H, kernel, stride, same_pad, store, kh, kw, cout, cin, ptr(bias), int(stride),
                      1 if same_pad else 0, store)


def tconv(w, x, x_store, x_bits, N, H, W, bn_inv=None, bn_shift=None, fn=FN_NONE, act_bits=0, out_store=STORE_F32,
          out=None, epilogue=None):
    """qnn_tconv_forward: x is a float32 NHWC CUDA tensor (x_store = STORE_F32) or int32 packed words as pack() writes
    them.  Returns (y, Ho, Wo): y float32 (N, Ho, Wo, Cout) or int32 (N * Ho * Wo, words).  `epilogue`: a ready Epilogue
    instead of the keyword fields (tests of the refusals).  A refusal with QNN_EUNSUPPORTED raises QnnUnsupported."""
    Ho, Wo = w.out_hw(H, W)
    return _side_forward("qnn_tconv", "tconv", w, x, x_store, x_bits, N, H, W, Ho, Wo, bn_inv, bn_shift, fn, act_bits,
                         out_store, out, epilogue)


def gconv_out_hw(size, k, stride, same_pad, dilation=1):
    """Output size of one axis of a grouped convolution: TensorFlow's rule on the effective window (csrc/qnn_conv_geom.h)."""
    return out_hw(size, k, stride, same_pad, dilation)


class GConvWeights(_SideWeights):
    """Owner of an opaque qnn_gconv_weights_t handle (include/qnn_abi_gconv.h).  kernel: float32 CUDA tensor in Keras'
    grouped layout (kh, kw, Cin / groups, Cout); bias: (Cout,) or None."""
    _prefix, _what = "qnn_gconv", "gconv"

    def __init__(self, wkind, wbits, H, kernel, bias, groups, stride, same_pad, store, dilation=(1, 1)):
        kernel, bias = self._tensors("(kh, kw, Cin / groups, Cout)", kernel, bias)
        kh, kw, cg, cout = kernel.shape
        groups = int(groups)
        if bias is not None and bias.numel() != cout:
            raise QnnError("gconv prepack: bias of %d values for %d filters" % (bias.numel(), cout))
        self.groups, self.cin, self.cout = groups, cg * groups, cout
        self.dilation = (int(dilation[0]), int(dilation[1]))
        self._prepack(wkind, wbits, H, kernel, stride, same_pad, store, kh, kw, self.cin, cout, groups, ptr(bias),
                      int(stride), 1 if same_pad else 0, self.dilation[0], self.dilation[1], store)


def gconv(w, x, x_store, x_bits, N, H, W, bn_inv=None, bn_shift=None, fn=FN_NONE, act_bits=0, out_store=STORE_F32,
          out=None, epilogue=None):
    """qnn_gconv_forward: x is a float32 NHWC CUDA tensor (x_store = STORE_F32) or int32 packed words as pack() writes
    them.  Returns (y, Ho, Wo): y float32 (N, Ho, Wo, Cout) or int32 (N * Ho * Wo, words).  `epilogue`: a ready Epilogue
    instead of the keyword fields (tests of the refusals).  A refusal with QNN_EUNSUPPORTED raises QnnUnsupported."""
    Ho, Wo = w.out_hw(H, W)
    _refuse_empty("gconv", w, H, W, Ho, Wo)
    return _side_forward("qnn_gconv", "gconv", w, x, x_store, x_bits, N, H, W, Ho, Wo, bn_inv, bn_shift, fn, act_bits,
                         out_store, out, epilogue)

