"""keras.layers.DepthwiseConv2D and its binary / quantized / ternary forms; forward through qnn_depthwise_forward
(include/qnn_abi_depthwise.h).  The reference has no depthwise layer: the low-bit classes take the constructor surface of
its conv layers (H, kernel_lr_multiplier, bias_lr_multiplier, nb) with Keras' depthwise arguments, and apply the same
weight quantisers elementwise to the depthwise kernel (kh, kw, C, depth_multiplier).  Output channel c * M + m reads input
channel c (Keras' order)."""
from .. import _abi
from ._base import LowBitLayer, _pair, glorot_H, glorot_lr_multiplier


class _DepthwiseBase(LowBitLayer):
    def _dw_init(self, H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, name):
        kwargs = dict(kwargs)
        if "kernel_size" not in kwargs:
            raise TypeError("__init__() missing 1 required positional argument: 'kernel_size'")
        self.kernel_size = _pair(kwargs.pop("kernel_size"))
        self.strides = _pair(kwargs.pop("strides", (1, 1)))
        self.padding = str(kwargs.pop("padding", "valid")).lower()
        self.depth_multiplier = int(kwargs.pop("depth_multiplier", 1))
        self.data_format = kwargs.pop("data_format", "channels_last") or "channels_last"
        self.dilation_rate = _pair(kwargs.pop("dilation_rate", (1, 1)))
        for keras_name, ours in (("depthwise_initializer", "kernel_initializer"),
                                 ("depthwise_regularizer", "kernel_regularizer"),
                                 ("depthwise_constraint", "kernel_constraint")):
            if keras_name in kwargs:
                kwargs[ours] = kwargs.pop(keras_name)
        kwargs = self._init_common(H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, name)
        if kwargs:
            raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))
        if self.padding not in ("same", "valid"):
            raise ValueError("The `padding` argument must be one of \"valid\", \"same\". Received: " + self.padding)
        if self.data_format != "channels_last":
            raise _abi.QnnError("only data_format='channels_last' (NHWC) is supported")
        if self.depth_multiplier < 1:
            raise ValueError("`depth_multiplier` must be a positive integer. Received: %d" % self.depth_multiplier)
        if min(self.kernel_size) < 1 or max(self.kernel_size) > _abi.DW_MAX_WINDOW:
            raise _abi.QnnError("kernel_size %s: depthwise windows are 1 .. %d per axis" % (self.kernel_size, _abi.DW_MAX_WINDOW))
        if self.dilation_rate != (1, 1) and self.strides != (1, 1):
            raise ValueError("`strides > 1` not supported in conjunction with `dilation_rate > 1`. Received: strides=%s "
                             "and dilation_rate=%s" % (self.strides, self.dilation_rate))
        if self.strides[0] != self.strides[1] or self.strides[0] not in (1, 2):
            raise _abi.QnnError("strides %s: square strides of 1 or 2 are supported" % (self.strides,))

    def build(self, input_shape):
        if input_shape[-1] is None:
            raise ValueError("The channel dimension of the inputs should be defined. Found `None`.")
        input_dim = int(input_shape[-1])
        base = self.kernel_size[0] * self.kernel_size[1]
        nb_input, nb_output = base, base * self.depth_multiplier      # fan-in / fan-out of one channel's filters
        if self.H == "Glorot":
            self.H = glorot_H(nb_input, nb_output)
        if self.kernel_lr_multiplier == "Glorot":
            self.kernel_lr_multiplier = glorot_lr_multiplier(nb_input, nb_output)
        self._init_weights(self.kernel_size + (input_dim, self.depth_multiplier), input_dim * self.depth_multiplier)
        self.input_dim = input_dim
        self.built = True

    def compute_output_shape(self, input_shape):
        n, h, w, c = input_shape
        same = self.padding == "same"
        return (n, _abi.out_hw(h, self.kernel_size[0], self.strides[0], same, self.dilation_rate[0]),
                _abi.out_hw(w, self.kernel_size[1], self.strides[1], same, self.dilation_rate[1]),
                c * self.depth_multiplier)

    def _weights(self, store):
        w = self._packed.get(store)
        if w is None:
            w = _abi.DepthwiseWeights(self._wkind, self._wbits(), float(self.H), self.kernel, self.bias, self.strides[0],
                                      self.padding == "same", store, dilation=self.dilation_rate)
            self._packed[store] = w
        return w

    def call(self, inputs):
        x = _abi.require_cuda(inputs, self.name + ".call")
        if x.dim() != 4 or x.shape[-1] != self.input_dim:
            raise ValueError("Input 0 is incompatible with layer %s: expected axis -1 of input shape to have value %d "
                             "but got shape %s" % (self.name, self.input_dim, tuple(x.shape)))
        N, H, W, C = x.shape
        plan = self._plan() if self._wkind != _abi.W_FLOAT else None
        if plan is None:
            y, _, _ = _abi.depthwise(self._weights(_abi.STORE_F32), x, _abi.STORE_F32, 0, N, H, W)
        else:
            store, bits, fn, nb = plan
            xp = _abi.pack(x, C, fn, nb, store)
            y, _, _ = _abi.depthwise(self._weights(store), xp, store, bits, N, H, W)
        if self.activation is not None:
            y = self.activation(y)
        return y

    def get_config(self):
        cfg = self._base_config()
        cfg.update({"kernel_size": self.kernel_size, "strides": self.strides, "padding": self.padding,
                    "depth_multiplier": self.depth_multiplier, "data_format": self.data_format,
                    "dilation_rate": self.dilation_rate})
        if self._wkind != _abi.W_FLOAT:
            cfg.update(self._own_config())
        return cfg

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class DepthwiseConv2D(_DepthwiseBase):
    """Stock keras.layers.DepthwiseConv2D: float32 weights used as they are."""

    _wkind = _abi.W_FLOAT

    def __init__(self, kernel_size, **kwargs):
        kwargs["kernel_size"] = kernel_size
        self._dw_init(1.0, None, None, kwargs, "depthwise_conv2d")


class BinaryDepthwiseConv2D(_DepthwiseBase):
    """depthwise_conv2d(x, binarize(W, H)) + b."""

    _wkind = _abi.W_BINARY

    def __init__(self, kernel_size, H=1., kernel_lr_multiplier='Glorot', bias_lr_multiplier=None, **kwargs):
        kwargs["kernel_size"] = kernel_size
        self._dw_init(H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, "binary_depthwise_conv2d")


class QuantizedDepthwiseConv2D(_DepthwiseBase):
    """depthwise_conv2d(x, quantize(W, nb)) + b."""

    _wkind = _abi.W_QUANT

    def __init__(self, kernel_size, H=1., nb=16, kernel_lr_multiplier='Glorot', bias_lr_multiplier=None, **kwargs):
        self.nb = int(nb)
        kwargs["kernel_size"] = kernel_size
        self._dw_init(H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, "quantized_depthwise_conv2d")


class TernaryDepthwiseConv2D(_DepthwiseBase):
    """depthwise_conv2d(x, ternarize(W, H)) + b; the cutoff 0.7 * mean|W / H| is taken over the depthwise kernel."""

    _wkind = _abi.W_TERNARY

    def __init__(self, kernel_size, H=1., kernel_lr_multiplier='Glorot', bias_lr_multiplier=None, **kwargs):
        kwargs["kernel_size"] = kernel_size
        self._dw_init(H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, "ternary_depthwise_conv2d")
