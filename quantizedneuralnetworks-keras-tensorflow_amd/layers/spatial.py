"""Keras' ZeroPadding2D, Cropping2D and UpSampling2D on the GPU (keras/layers/convolutional.py of Keras 2.1.3,
channels_last): float32 NHWC in, float32 NHWC out, through qnn_spatial2d_forward (include/qnn_abi_spatial.h).  Every output
pixel is a copy of one input pixel or zero.  The engines run the same entry on packed codes (engine.py)."""
from .. import _abi
from .pooling import _nhwc


def _channels_last(data_format):
    data_format = data_format or "channels_last"
    if data_format not in ("channels_last", "channels_first"):
        raise ValueError("The `data_format` argument must be one of \"channels_first\", \"channels_last\". Received: "
                         + str(data_format))
    if data_format != "channels_last":
        raise ValueError("only data_format='channels_last' (NHWC) is supported")
    return data_format


class _Spatial2D:
    """One step of qnn_spatial2d_t: the subclass says which (`_field`) and reads its Keras argument."""
    _field = None

    def _init(self, data_format, name, kwargs):
        kwargs.pop("input_shape", None)
        kwargs.pop("trainable", None)
        if kwargs:
            raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))
        self.data_format = _channels_last(data_format)
        self.name = name or type(self).__name__.lower()

    def _steps(self):
        return {self._field: getattr(self, self._attr)}

    def compute_output_shape(self, input_shape):
        n, h, w, c = input_shape
        if h is None or w is None:
            raise ValueError("%s: the rows and columns of the input must be known" % self.name)
        return (n,) + _abi.spatial2d_out_hw(h, w, **self._steps()) + (c,)

    def call(self, inputs):
        x = _nhwc(inputs, self.name)
        N, H, W, C = x.shape
        return _abi.spatial2d(x, _abi.STORE_F32, 0, N, H, W, C, **self._steps())[0]

    __call__ = call

    def get_config(self):
        return {"name": self.name, "trainable": True, self._attr: getattr(self, self._attr), "data_format": self.data_format}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class ZeroPadding2D(_Spatial2D):
    """keras.layers.ZeroPadding2D(padding=(1, 1), data_format=None): an int, (rows, columns) or ((top, bottom), (left, right))"""
    _field, _attr = "pad", "padding"

    def __init__(self, padding=(1, 1), data_format=None, name=None, **kwargs):
        self._init(data_format, name, kwargs)
        t, b, l, r = _abi.pairs2d(padding, "padding")
        if min(t, b, l, r) < 0:
            raise ValueError("`padding` must not be negative. Received: %r" % (padding,))
        self.padding = ((t, b), (l, r))


class Cropping2D(_Spatial2D):
    """keras.layers.Cropping2D(cropping=((0, 0), (0, 0)), data_format=None): an int, (rows, columns) or ((top, bottom), (left, right))"""
    _field, _attr = "crop", "cropping"

    def __init__(self, cropping=((0, 0), (0, 0)), data_format=None, name=None, **kwargs):
        self._init(data_format, name, kwargs)
        t, b, l, r = _abi.pairs2d(cropping, "cropping")
        if min(t, b, l, r) < 0:
            raise ValueError("`cropping` must not be negative. Received: %r" % (cropping,))
        self.cropping = ((t, b), (l, r))


class UpSampling2D(_Spatial2D):
    """keras.layers.UpSampling2D(size=(2, 2), data_format=None): every row repeated size[0] times, every column size[1]
    times (nearest neighbour, the only form Keras 2.1.3 has)."""
    _field, _attr = "up", "size"

    def __init__(self, size=(2, 2), data_format=None, interpolation="nearest", name=None, **kwargs):
        self._init(data_format, name, kwargs)
        if interpolation != "nearest":
            raise ValueError("UpSampling2D: interpolation=%r; only 'nearest' is supported (Keras 2.1.3 has no other)"
                             % (interpolation,))
        self.size = _abi._pair(size, "size")
        if min(self.size) < 1:
            raise ValueError("`size` must be positive. Received: %r" % (size,))
