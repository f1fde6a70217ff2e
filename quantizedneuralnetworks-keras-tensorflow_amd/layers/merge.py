"""Keras' Concatenate on the GPU (keras/layers/merge.py of Keras 2.1.3, channels_last): a list of float32 tensors in,
their concatenation along the channels out, through qnn_concat_forward (include/qnn_abi_concat.h).  The engines run the
same entry on packed codes (engine.py)."""
from .. import _abi


class Concatenate:
    """keras.layers.Concatenate(axis=-1): the channel axis only (the last one of an NHWC or an (N, K) tensor)."""

    def __init__(self, axis=-1, name=None, **kwargs):
        kwargs.pop("input_shape", None)
        kwargs.pop("trainable", None)
        if kwargs:
            raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))
        self.axis = int(axis)
        self.name = name or type(self).__name__.lower()

    def _check(self, shapes):
        """Keras' own checks (merge.py:Concatenate.build), then the axis this port has a kernel for."""
        if not isinstance(shapes, (list, tuple)) or len(shapes) < 2 or not all(isinstance(s, (list, tuple)) for s in shapes):
            raise ValueError("A `Concatenate` layer should be called on a list of at least 2 inputs")
        shapes = [tuple(s) for s in shapes]
        rank = len(shapes[0])
        if any(len(s) != rank for s in shapes) or rank not in (2, 4):
            raise ValueError("A `Concatenate` layer requires inputs with matching shapes except for the concat axis. "
                             "Got inputs shapes: %s" % (shapes,))
        if self.axis not in (-1, rank - 1):
            raise _abi.QnnError("%s: axis=%d of rank-%d inputs; only the channel axis (-1 or %d) is supported"
                                % (self.name, self.axis, rank, rank - 1))
        if len({s[:-1] for s in shapes}) > 1:
            raise ValueError("A `Concatenate` layer requires inputs with matching shapes except for the concat axis. "
                             "Got inputs shapes: %s" % (shapes,))
        return shapes

    def compute_output_shape(self, input_shape):
        shapes = self._check(input_shape)
        last = [s[-1] for s in shapes]
        return shapes[0][:-1] + (None if any(c is None for c in last) else sum(last),)

    def call(self, inputs):
        if not isinstance(inputs, (list, tuple)) or len(inputs) < 2:
            raise ValueError("A `Concatenate` layer should be called on a list of at least 2 inputs")
        shapes = self._check([tuple(x.shape) for x in inputs])      # the shapes first: these answers need no device
        xs = [_abi.require_cuda(x, self.name) for x in inputs]
        lead = shapes[0][:-1]
        pixels = 1
        for d in lead:
            pixels *= d
        channels = [s[-1] for s in shapes]
        y = _abi.concat(xs, channels, _abi.STORE_F32, 0, pixels)
        return y.reshape(lead + (sum(channels),))

    __call__ = call

    def get_config(self):
        return {"name": self.name, "trainable": True, "axis": self.axis}

    @classmethod
    def from_config(cls, config):
        return cls(**config)
