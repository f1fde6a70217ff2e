"""Counterparts of the reference's layers/quantized_ops.py (forward only)."""
import torch

from .. import _abi


def quantized_tanh(W, nb=16):
    """quantized_ops.py:87-100: clip(round(W*m), -m, m-1)/m, m = 2**(nb-1).
    This is the activation the models use (model_factory.py:9,19-20)."""
    W = _abi.require_cuda(W, "quantized_tanh")
    y = torch.empty_like(W)
    _abi.check(_abi.load().qnn_quantized_tanh_f32(_abi.ptr(W), _abi.ptr(y), W.numel(), int(nb),
                                                  _abi.stream_ptr()), "quantized_tanh")
    return y


def _quantized_act(W, fn, nb, what):
    W = _abi.require_cuda(W, what)
    y = torch.empty_like(W)
    _abi.check(_abi.load().qnn_quantized_act_f32(_abi.ptr(W), _abi.ptr(y), W.numel(), fn, int(nb), _abi.stream_ptr()), what)
    return y


def quantized_relu(W, nb=16):
    """quantized_ops.py:69-84: clip(2*round(hard_sigmoid(W)*2**nb)/2**nb - 1, 0, 1 - 1/m), m = 2**(nb-1).  Only W + 1
    rounds, so this is clip(round((W + 1)*m) - m, 0, m - 1)/m -- not quantized_tanh clamped at 0 (include/qnn_abi.h)."""
    return _quantized_act(W, _abi.FN_QUANTIZED_RELU, nb, "quantized_relu")


LEAKY_ALPHA = 0.1


def quantized_leakyrelu(W, nb=16, alpha=LEAKY_ALPHA):
    """quantized_ops.py:102-123: quantized_tanh of (W >= 0 ? W : float32(alpha) * W).  The kernels carry the reference's
    default alpha = float32(0.1) only (as LeakyReLU is fixed at 0.3): any other alpha raises ValueError."""
    check_leaky_alpha(alpha)
    return _quantized_act(W, _abi.FN_QUANTIZED_LEAKYRELU, nb, "quantized_leakyrelu")


def check_leaky_alpha(alpha, what="quantized_leakyrelu"):
    import numpy as np
    if np.float32(alpha) != np.float32(LEAKY_ALPHA):
        raise ValueError("%s: only alpha = %r (the reference's default) is supported, got %r"
                         % (what, LEAKY_ALPHA, alpha))


def _quantized_maxact(W, fn, nb, group, what):
    """The reduction kernel, the all-reduce of its word between the halves of a sharded batch, the apply kernel -- built
    like ternary_ops.ternary_tanh.  Nothing is read back to the host."""
    W = _abi.require_cuda(W, what)
    y = torch.empty_like(W)
    ws = maxact_word(W, group, what)
    _abi.check(_abi.load().qnn_maxact_apply_f32(_abi.ptr(W), _abi.ptr(y), W.numel(), fn, int(nb), _abi.ptr(ws),
                                                _abi.stream_ptr()), what)
    return y


def maxact_word(W, group=None, what="maxact_word"):
    """Pass 1 of the two activations on the contiguous float32 CUDA tensor W: a fresh 16-byte workspace (int32[4]) whose
    first word holds the bits of the maximum -- of the valid rows under `shard.sharded(..., valid_rows=k)`, all-reduced
    between the shards.  The apply pass and the pack pass (include/qnn_abi_scaled.h) and every scaled consumer read it."""
    from .. import shard
    ws = torch.empty(4, dtype=torch.int32, device=W.device)          # the 16-byte workspace: word 0 = bits(M)
    n_max = W.numel()
    valid = shard.active_valid_rows()
    if valid is not None and W.dim() >= 1 and W.shape[0] > 0:
        n_max = min(int(valid), W.shape[0]) * (W.numel() // W.shape[0])
    _abi.check(_abi.load().qnn_maxact_max_f32(_abi.ptr(W), n_max, _abi.ptr(ws), _abi.stream_ptr()), what)
    shard.allreduce_max(ws, group)
    return ws


def quantized_maxrelu(W, nb=16, group=None):
    """quantized_ops.py:125-143, by the exact rule of include/qnn_abi_maxact.h: M = max(W, 0) over the WHOLE tensor, P =
    the smallest power of two >= M (from M's exponent and mantissa bits, no log), m = 2**(nb-1), nb in 2 .. 24:
    clip(rint(W * (m / P)), 0, m - 1) * (P / m), one rounding (the rint, half to even) per value.

    The maximum is per batch TENSOR: predict(batch_size=b) scales each batch by its own maximum, as the reference's
    predict does.  When the batch is sharded over processes (`shard.sharded(...)` is active, or `group` is given) the
    maximum is all-reduced between the reduction kernel and the apply kernel; a shard padded to the common size
    (`shard.sharded(group, valid_rows=k)`) contributes only its first k batch rows to it.
    No positive value (M <= 0, where the reference takes the log of zero), or M outside (2**-65, 2**64]: every output
    element is NaN; nothing is read back, synchronised or raised.

    Deviation from the reference: it computes the exponent as ceil(log(M) / log(2)) in float32.  Where M is an exact
    power of two or lies within 16 ulp above one, that quotient may be one off the exact value, depending on the
    platform's float32 log, and the reference's scale is then 2x or 1/2x this one.  This op always takes the exact value."""
    return _quantized_maxact(W, _abi.FN_QUANTIZED_MAXRELU, nb, group, "quantized_maxrelu")


def quantized_leakymaxrelu(W, nb=16, alpha=LEAKY_ALPHA, group=None):
    """quantized_ops.py:145-171: quantized_maxrelu's scale (the maximum is that of the positive values) applied to
    L(W) = (W >= 0 ? W : float32(alpha) * W) with the clip [-m, m - 1].  Range, sharding, NaN rule and the deviation band:
    see quantized_maxrelu.  As quantized_leakyrelu, the kernels carry alpha = float32(0.1) only: any other raises
    ValueError."""
    check_leaky_alpha(alpha, "quantized_leakymaxrelu")
    return _quantized_maxact(W, _abi.FN_QUANTIZED_LEAKYMAXRELU, nb, group, "quantized_leakymaxrelu")


def quantize(W, nb=16, clip_through=False):
    """quantized_ops.py:49-66.  `clip_through` only changes the gradient."""
    return quantized_tanh(W, nb)
