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


class _Merge:
    """keras.layers.merge._Merge for tensors of one shape: a list of float32 tensors in, `fn` of them out, element by
    element, through qnn_merge_forward (include/qnn_abi_merge.h): Keras' own left-to-right chain, one rounding per step.
    Keras broadcasts inputs of different shapes; this port does not (QnnError naming the shapes)."""

    fn = None

    def __init__(self, name=None, **kwargs):
        kwargs.pop("input_shape", None)
        kwargs.pop("trainable", None)
        if kwargs:
            raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))
        self.name = name or type(self).__name__.lower()

    def _check(self, shapes):
        """Keras' own checks (merge.py:_Merge.build), then the one shape this port has a kernel for."""
        if not isinstance(shapes, (list, tuple)) or (shapes and not all(isinstance(s, (list, tuple)) for s in shapes)):
            raise ValueError("A merge layer should be called on a list of inputs.")
        if len(shapes) < 2:
            raise ValueError("A merge layer should be called on a list of at least 2 inputs. Got %d inputs." % len(shapes))
        if self.fn == "sub" and len(shapes) != 2:
            raise ValueError("A `Subtract` layer should be called on exactly 2 inputs")
        shapes = [tuple(s) for s in shapes]
        if len(set(shapes)) != 1:
            raise _abi.QnnError("%s: inputs of shapes %s; only identical shapes are supported (no broadcasting)"
                                % (self.name, shapes))
        if len(shapes) > _abi.MERGE_MAX:
            raise _abi.QnnError("%s: %d inputs (at most %d)" % (self.name, len(shapes), _abi.MERGE_MAX))
        return shapes

    def compute_output_shape(self, input_shape):
        return self._check(input_shape)[0]

    def call(self, inputs):
        if not isinstance(inputs, (list, tuple)):
            raise ValueError("A merge layer should be called on a list of inputs.")
        shape = self._check([tuple(x.shape) for x in inputs])[0]      # the shapes first: these answers need no device
        xs = [_abi.require_cuda(x, self.name) for x in inputs]
        if not shape:
            raise _abi.QnnError("%s: scalar inputs" % self.name)
        pixels = 1
        for d in shape[:-1]:
            pixels *= d
        return _abi.merge(xs, self.fn, _abi.STORE_F32, 0, pixels, shape[-1])[0].reshape(shape)

    __call__ = call

    def get_config(self):
        return {"name": self.name, "trainable": True}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class Add(_Merge):
    """keras.layers.Add: x0 + x1 + ... left to right."""
    fn = "add"


class Subtract(_Merge):
    """keras.layers.Subtract: x0 - x1, exactly two inputs."""
    fn = "sub"


class Multiply(_Merge):
    """keras.layers.Multiply: x0 * x1 * ... left to right."""
    fn = "mul"


class Average(_Merge):
    """keras.layers.Average: the sum chain of Add, then one division by the number of inputs."""
    fn = "avg"


class Maximum(_Merge):
    """keras.layers.Maximum: element-wise maximum; NaN where any input is NaN."""
    fn = "max"


class Minimum(_Merge):
    """keras.layers.Minimum: element-wise minimum; NaN where any input is NaN."""
    fn = "min"
