"""Keras' pooling layers on the GPU: MaxPooling2D, AveragePooling2D, GlobalAveragePooling2D, GlobalMaxPooling2D
(keras/layers/pooling.py of Keras 2.1.3, channels_last), float32 NHWC in, float32 out, through qnn_pool2d_forward
(include/qnn_abi_pool.h).  'same' padding is TensorFlow's: it takes no part in a maximum and is not counted by an
average.  The engines run the same entry on packed codes (engine.py)."""
from .. import _abi


def _conv_pair(value, name):
    """keras.utils.conv_utils.normalize_tuple(value, 2, name)"""
    if isinstance(value, int):
        return (value, value)
    try:
        t = tuple(value)
    except TypeError:
        t = None
    if t is None or len(t) != 2 or not all(isinstance(v, int) for v in t):
        raise ValueError("The `%s` argument must be a tuple of 2 integers. Received: %s" % (name, value))
    return t


def _data_format(data_format):
    data_format = data_format or "channels_last"
    if data_format not in ("channels_last", "channels_first"):
        raise ValueError("The `data_format` argument must be one of \"channels_first\", \"channels_last\". Received: "
                         + str(data_format))
    if data_format != "channels_last":
        raise _abi.QnnError("only data_format='channels_last' (NHWC) is supported")
    return data_format


def _nhwc(x, what):
    x = _abi.require_cuda(x, what)
    if x.dim() != 4:
        raise ValueError("Input 0 is incompatible with layer %s: expected ndim=4, found ndim=%d" % (what, x.dim()))
    return x


class _Pooling2D:
    _mode = None

    def __init__(self, pool_size=(2, 2), strides=None, padding="valid", data_format=None, name=None, **kwargs):
        kwargs.pop("input_shape", None)
        kwargs.pop("trainable", None)
        if kwargs:
            raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))
        self.pool_size = _conv_pair(pool_size, "pool_size")
        self.strides = _conv_pair(self.pool_size if strides is None else strides, "strides")
        self.padding = str(padding).lower()
        if self.padding not in ("same", "valid"):
            raise ValueError("The `padding` argument must be one of \"valid\", \"same\". Received: " + self.padding)
        if min(self.pool_size + self.strides) < 1:
            raise ValueError("`pool_size` and `strides` must be positive. Received: pool_size=%s strides=%s"
                             % (self.pool_size, self.strides))
        self.data_format = _data_format(data_format)
        self.name = name or type(self).__name__.lower()

    def compute_output_shape(self, input_shape):
        n, h, w, c = input_shape
        same = self.padding == "same"
        rows = None if h is None else _abi.out_hw(h, self.pool_size[0], self.strides[0], same, 1)
        cols = None if w is None else _abi.out_hw(w, self.pool_size[1], self.strides[1], same, 1)
        return (n, rows, cols, c)

    def call(self, inputs):
        x = _nhwc(inputs, self.name)
        N, H, W, C = x.shape
        return _abi.pool2d(x, _abi.STORE_F32, 0, N, H, W, C, self._mode, self.pool_size, self.strides,
                           self.padding == "same")[0]

    __call__ = call

    def get_config(self):
        return {"name": self.name, "trainable": True, "pool_size": self.pool_size, "padding": self.padding,
                "strides": self.strides, "data_format": self.data_format}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class MaxPooling2D(_Pooling2D):
    """keras.layers.MaxPooling2D(pool_size=(2, 2), strides=None, padding='valid', data_format=None)"""
    _mode = _abi.POOL_MAX


class AveragePooling2D(_Pooling2D):
    """keras.layers.AveragePooling2D(pool_size=(2, 2), strides=None, padding='valid', data_format=None)"""
    _mode = _abi.POOL_AVG


class _GlobalPooling2D:
    _mode = None

    def __init__(self, data_format=None, name=None, **kwargs):
        kwargs.pop("input_shape", None)
        kwargs.pop("trainable", None)
        if kwargs:
            raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))
        self.data_format = _data_format(data_format)
        self.name = name or type(self).__name__.lower()

    def compute_output_shape(self, input_shape):
        return (input_shape[0], input_shape[3])

    def call(self, inputs):
        x = _nhwc(inputs, self.name)
        N, H, W, C = x.shape
        return _abi.pool2d(x, _abi.STORE_F32, 0, N, H, W, C, self._mode, (H, W))[0].reshape(N, C)

    __call__ = call

    def get_config(self):
        return {"name": self.name, "trainable": True, "data_format": self.data_format}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class GlobalAveragePooling2D(_GlobalPooling2D):
    """keras.layers.GlobalAveragePooling2D(data_format=None): the mean over rows and columns, (N, C)"""
    _mode = _abi.POOL_AVG


class GlobalMaxPooling2D(_GlobalPooling2D):
    """keras.layers.GlobalMaxPooling2D(data_format=None): the maximum over rows and columns, (N, C)"""
    _mode = _abi.POOL_MAX
