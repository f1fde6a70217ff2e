"""keras.layers.Conv2DTranspose and its binary / quantized / ternary forms; forward through qnn_tconv_forward
(include/qnn_abi_tconv.h).  The reference has no transposed convolution: the low-bit classes take the constructor surface
of its conv layers (H, kernel_lr_multiplier, bias_lr_multiplier, nb) with Keras' Conv2DTranspose arguments, and apply the
same weight quantisers elementwise to the kernel, which is Keras' (kh, kw, filters, Cin): filters before input channels."""
from .. import _abi
from ._base import LowBitLayer, _pair, glorot_H, glorot_lr_multiplier


class _TransposeBase(LowBitLayer):
    def _tc_init(self, H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, name):
        kwargs = dict(kwargs)
        for required in ("filters", "kernel_size"):
            if required not in kwargs:
                raise TypeError("__init__() missing 1 required positional argument: %r" % required)
        self.filters = int(kwargs.pop("filters"))
        self.kernel_size = _pair(kwargs.pop("kernel_size"))
        self.strides = _pair(kwargs.pop("strides", (1, 1)))
        self.padding = str(kwargs.pop("padding", "valid")).lower()
        self.output_padding = kwargs.pop("output_padding", None)
        self.data_format = kwargs.pop("data_format", "channels_last") or "channels_last"
        self.dilation_rate = _pair(kwargs.pop("dilation_rate", (1, 1)))
        kwargs = self._init_common(H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, name)
        if kwargs:
            raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))
        if self.filters < 1:
            raise ValueError("`filters` must be a positive integer. Received: %d" % self.filters)
        if self.padding not in ("same", "valid"):
            raise ValueError("The `padding` argument must be one of \"valid\", \"same\". Received: " + self.padding)
        if self.data_format != "channels_last":
            raise _abi.QnnError("only data_format='channels_last' (NHWC) is supported")
        if self.output_padding is not None:
            raise _abi.QnnError("output_padding=%r: only None is supported" % (self.output_padding,))
        if self.dilation_rate != (1, 1):
            raise _abi.QnnError("dilation_rate=%s: a transposed convolution supports (1, 1) only" % (self.dilation_rate,))
        if min(self.kernel_size) < 1 or max(self.kernel_size) > _abi.TC_MAX_WINDOW:
            raise _abi.QnnError("kernel_size %s: transposed windows are 1 .. %d per axis" % (self.kernel_size, _abi.TC_MAX_WINDOW))
        if self.strides[0] != self.strides[1] or not 1 <= self.strides[0] <= _abi.TC_MAX_STRIDE:
            raise _abi.QnnError("strides %s: square strides of 1 .. %d are supported" % (self.strides, _abi.TC_MAX_STRIDE))

    def build(self, input_shape):
        if input_shape[-1] is None:
            raise ValueError("The channel dimension of the inputs should be defined. Found `None`.")
        input_dim = int(input_shape[-1])
        base = self.kernel_size[0] * self.kernel_size[1]
        nb_input, nb_output = int(input_dim * base), int(self.filters * base)
        if self.H == "Glorot":
            self.H = glorot_H(nb_input, nb_output)
        if self.kernel_lr_multiplier == "Glorot":
            self.kernel_lr_multiplier = glorot_lr_multiplier(nb_input, nb_output)
        self._init_weights(self.kernel_size + (self.filters, input_dim), self.filters)
        self.input_dim = input_dim
        self.built = True

    def compute_output_shape(self, input_shape):
        n, h, w, _ = input_shape
        same = self.padding == "same"
        return (n, _abi.tconv_out_hw(h, self.kernel_size[0], self.strides[0], same),
                _abi.tconv_out_hw(w, self.kernel_size[1], self.strides[1], same), self.filters)

    def _weights(self, store):
        w = self._packed.get(store)
        if w is None:
            w = _abi.TConvWeights(self._wkind, self._wbits(), float(self.H), self.kernel, self.bias, self.strides[0],
                                  self.padding == "same", store)
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
            y, _, _ = _abi.tconv(self._weights(_abi.STORE_F32), x, _abi.STORE_F32, 0, N, H, W)
        else:
            store, bits, fn, nb = plan
            xp = _abi.pack(x, C, fn, nb, store)
            y, _, _ = _abi.tconv(self._weights(store), xp, store, bits, N, H, W)
        if self.activation is not None:
            y = self.activation(y)
        return y

    def get_config(self):
        cfg = self._base_config()
        cfg.update({"filters": self.filters, "kernel_size": self.kernel_size, "strides": self.strides,
                    "padding": self.padding, "output_padding": self.output_padding, "data_format": self.data_format,
                    "dilation_rate": self.dilation_rate})
        if self._wkind != _abi.W_FLOAT:
            cfg.update(self._own_config())
        return cfg

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class Conv2DTranspose(_TransposeBase):
    """Stock keras.layers.Conv2DTranspose: float32 weights used as they are."""

    _wkind = _abi.W_FLOAT

    def __init__(self, filters, kernel_size, **kwargs):
        kwargs.update(filters=filters, kernel_size=kernel_size)
        self._tc_init(1.0, None, None, kwargs, "conv2d_transpose")


class BinaryConv2DTranspose(_TransposeBase):
    """conv2d_transpose(x, binarize(W, H)) + b."""

    _wkind = _abi.W_BINARY

    def __init__(self, filters, kernel_size, H=1., kernel_lr_multiplier='Glorot', bias_lr_multiplier=None, **kwargs):
        kwargs.update(filters=filters, kernel_size=kernel_size)
        self._tc_init(H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, "binary_conv2d_transpose")


class QuantizedConv2DTranspose(_TransposeBase):
    """conv2d_transpose(x, quantize(W, nb)) + b."""

    _wkind = _abi.W_QUANT

    def __init__(self, filters, kernel_size, H=1., nb=16, kernel_lr_multiplier='Glorot', bias_lr_multiplier=None, **kwargs):
        self.nb = int(nb)
        kwargs.update(filters=filters, kernel_size=kernel_size)
        self._tc_init(H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, "quantized_conv2d_transpose")


class TernaryConv2DTranspose(_TransposeBase):
    """conv2d_transpose(x, ternarize(W, H)) + b; the cutoff 0.7 * mean|W / H| is taken over the whole kernel."""

    _wkind = _abi.W_TERNARY

    def __init__(self, filters, kernel_size, H=1., kernel_lr_multiplier='Glorot', bias_lr_multiplier=None, **kwargs):
        kwargs.update(filters=filters, kernel_size=kernel_size)
        self._tc_init(H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, "ternary_conv2d_transpose")
