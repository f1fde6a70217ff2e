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


def check_leaky_alpha(alpha):
    import numpy as np
    if np.float32(alpha) != np.float32(LEAKY_ALPHA):
        raise ValueError("quantized_leakyrelu: only alpha = %r (the reference's default) is supported, got %r"
                         % (LEAKY_ALPHA, alpha))


def quantize(W, nb=16, clip_through=False):
    """quantized_ops.py:49-66.  `clip_through` only changes the gradient."""
    return quantized_tanh(W, nb)
