"""keras.layers.Conv2D(..., groups=g) and its binary / quantized / ternary forms; forward through qnn_gconv_forward
(include/qnn_abi_gconv.h).  The reference's conv layers have no `groups`: these classes take their constructor surface (H,
kernel_lr_multiplier, bias_lr_multiplier, nb) plus Keras' `groups`, and apply the same weight quantisers elementwise to the
grouped kernel (kh, kw, Cin / groups, filters).  Filter f belongs to group f // (filters / groups) and reads that group's
Cin / groups input channels only."""
from .. import _abi
from ._base import LowBitLayer, _pair, glorot_H, glorot_lr_multiplier


class _GroupedBase(LowBitLayer):
    def _gc_init(self, H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, name):
        kwargs = dict(kwargs)
        for required in ("filters", "kernel_size"):
            if required not in kwargs:
                raise TypeError("__init__() missing 1 required positional argument: %r" % required)
        self.filters = int(kwargs.pop("filters"))
        self.kernel_size = _pair(kwargs.pop("kernel_size"))
        self.strides = _pair(kwargs.pop("strides", (1, 1)))
        self.padding = str(kwargs.pop("padding", "valid")).lower()
        self.data_format = kwargs.pop("data_format", "channels_last") or "channels_last"
        self.dilation_rate = _pair(kwargs.pop("dilation_rate", (1, 1)))
        self.groups = int(kwargs.pop("groups", 1))
        kwargs = self._init_common(H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, name)
        if kwargs:
            raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))
        if self.filters < 1:
            raise ValueError("`filters` must be a positive integer. Received: %d" % self.filters)
        if self.groups < 1:
            raise ValueError("The number of groups must be a positive integer. Received: groups=%d" % self.groups)
        if self.padding not in ("same", "valid"):
            raise ValueError("The `padding` argument must be one of \"valid\", \"same\". Received: " + self.padding)
        if self.data_format != "channels_last":
            raise _abi.QnnError("only data_format='channels_last' (NHWC) is supported")
        if min(self.kernel_size) < 1 or max(self.kernel_size) > _abi.GC_MAX_WINDOW:
            raise _abi.QnnError("kernel_size %s: grouped windows are 1 .. %d per axis" % (self.kernel_size, _abi.GC_MAX_WINDOW))
        if self.dilation_rate != (1, 1) and self.strides != (1, 1):
            raise ValueError("`strides > 1` not supported in conjunction with `dilation_rate > 1`. Received: strides=%s "
                             "and dilation_rate=%s" % (self.strides, self.dilation_rate))
        if self.strides[0] != self.strides[1] or self.strides[0] not in (1, 2):
            raise _abi.QnnError("strides %s: square strides of 1 or 2 are supported" % (self.strides,))

    def build(self, input_shape):
        if input_shape[-1] is None:
            raise ValueError("The channel dimension of the inputs should be defined. Found `None`.")
        input_dim = int(input_shape[-1])
        if self.filters % self.groups != 0:
            raise ValueError("The number of filters must be evenly divisible by the number of groups. Received: groups=%d, "
                             "filters=%d" % (self.groups, self.filters))
        if input_dim % self.groups != 0:
            raise ValueError("The number of input channels must be evenly divisible by the number of groups. Received "
                             "groups=%d, but the input has %d channels (full input shape is %s)."
                             % (self.groups, input_dim, tuple(input_shape)))
        base = self.kernel_size[0] * self.kernel_size[1]
        cg, fg = input_dim // self.groups, self.filters // self.groups
        nb_input, nb_output = int(cg * base), int(fg * base)         # fan-in / fan-out of one group
        if self.H == "Glorot":
            self.H = glorot_H(nb_input, nb_output)
        if self.kernel_lr_multiplier == "Glorot":
            self.kernel_lr_multiplier = glorot_lr_multiplier(nb_input, nb_output)
        self._init_weights(self.kernel_size + (cg, self.filters), self.filters)
        self.input_dim = input_dim
        self.built = True

    def compute_output_shape(self, input_shape):
        n, h, w, _ = input_shape
        same = self.padding == "same"
        return (n, _abi.gconv_out_hw(h, self.kernel_size[0], self.strides[0], same, self.dilation_rate[0]),
                _abi.gconv_out_hw(w, self.kernel_size[1], self.strides[1], same, self.dilation_rate[1]), self.filters)

    def _weights(self, store):
        w = self._packed.get(store)
        if w is None:
            w = _abi.GConvWeights(self._wkind, self._wbits(), float(self.H), self.kernel, self.bias, self.groups,
                                  self.strides[0], self.padding == "same", store, dilation=self.dilation_rate)
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
            y, _, _ = _abi.gconv(self._weights(_abi.STORE_F32), x, _abi.STORE_F32, 0, N, H, W)
        else:
            store, bits, fn, nb = plan
            xp = _abi.pack(x, C, fn, nb, store)
            y, _, _ = _abi.gconv(self._weights(store), xp, store, bits, N, H, W)
        if self.activation is not None:
            y = self.activation(y)
        return y

    def get_config(self):
        cfg = self._base_config()
        cfg.update({"filters": self.filters, "kernel_size": self.kernel_size, "strides": self.strides,
                    "padding": self.padding, "data_format": self.data_format, "dilation_rate": self.dilation_rate,
                    "groups": self.groups})
        if self._wkind != _abi.W_FLOAT:
            cfg.update(self._own_config())
        return cfg

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class GroupedConv2D(_GroupedBase):
    """Stock keras.layers.Conv2D with `groups`: float32 weights used as they are."""

    _wkind = _abi.W_FLOAT

    def __init__(self, filters, kernel_size, **kwargs):
        kwargs.update(filters=filters, kernel_size=kernel_size)
        self._gc_init(1.0, None, None, kwargs, "grouped_conv2d")


class BinaryGroupedConv2D(_GroupedBase):
    """grouped_conv2d(x, binarize(W, H)) + b."""

    _wkind = _abi.W_BINARY

    def __init__(self, filters, kernel_size, H=1., kernel_lr_multiplier='Glorot', bias_lr_multiplier=None, **kwargs):
        kwargs.update(filters=filters, kernel_size=kernel_size)
        self._gc_init(H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, "binary_grouped_conv2d")


class QuantizedGroupedConv2D(_GroupedBase):
    """grouped_conv2d(x, quantize(W, nb)) + b."""

    _wkind = _abi.W_QUANT

    def __init__(self, filters, kernel_size, H=1., nb=16, kernel_lr_multiplier='Glorot', bias_lr_multiplier=None, **kwargs):
        self.nb = int(nb)
        kwargs.update(filters=filters, kernel_size=kernel_size)
        self._gc_init(H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, "quantized_grouped_conv2d")


class TernaryGroupedConv2D(_GroupedBase):
    """grouped_conv2d(x, ternarize(W, H)) + b; the cutoff 0.7 * mean|W / H| is taken over the whole grouped kernel."""

    _wkind = _abi.W_TERNARY

    def __init__(self, filters, kernel_size, H=1., kernel_lr_multiplier='Glorot', bias_lr_multiplier=None, **kwargs):
        kwargs.update(filters=filters, kernel_size=kernel_size)
        self._gc_init(H, kernel_lr_multiplier, bias_lr_multiplier, kwargs, "ternary_grouped_conv2d")
