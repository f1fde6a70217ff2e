#!/usr/bin/env python3
"""Reference vectors for quantized_relu and quantized_leakyrelu: tests/golden/ref_qrelu.npz.

    python tests/golden/make_fixtures_qrelu.py [/root/reference]

For the build container only (the reference checkout is not part of this repository, and no test runs this file).  It
EXECUTES the reference's own layers/quantized_ops.py, imported from where it lies, on float32 numpy arrays: `keras.backend`
and `tensorflow` are replaced by the few eager float32 operations those two functions call (clip, round = half to even,
stop_gradient = identity, relu, cast / convert_to_tensor = one rounding to float32) -- the stand-in of
make_fixtures_from_reference.py has no tf.cast and no dtype.base_dtype, which quantized_leakyrelu asks for, so this file
carries a small one of its own.  The op sequence, the constants and their order are the reference's; nothing of its text
is copied here.

Inputs per nb in {2, 3, 4, 8} (m = 2^(nb-1)):
  every tie (k + 1/2)/m of quantized_leakyrelu's positive side and (k + 1/2)/m - 1 of quantized_relu's v + 1, the ties
  of the leaky side 10 (k + 1/2)/m, and the float32 neighbours of all of them;  +-0, +-2^-24, +-2^-25;  both clip edges
  (+-1, 1 - 1/m, -10) +- 1 ulp;  10^5 uniform values in [-1.5, 1.5].
Arrays: x_edges_nb<nb> and x_uniform (the input of width nb is their concatenation), relu_nb<nb>, leaky_nb<nb> (alpha = the
reference's default 0.1) -- the outputs as the reference returned them, float32.
"""
import os
import sys
import types

import numpy as np

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
NBS = (2, 3, 4, 8)


class _DType:
    base_dtype = np.float32


class Tensor:
    """Eager float32 tensor; a Python scalar meeting it is converted to float32 first (tf.convert_to_tensor)."""
    __array_priority__ = 1000.0
    dtype = _DType()

    def __init__(self, a):
        self.a = np.ascontiguousarray(np.asarray(a), dtype=np.float32)

    @staticmethod
    def _v(o):
        return o.a if isinstance(o, Tensor) else np.asarray(o, dtype=np.float32)

    def __add__(self, o): return Tensor(self.a + self._v(o))
    def __radd__(self, o): return Tensor(self._v(o) + self.a)
    def __sub__(self, o): return Tensor(self.a - self._v(o))
    def __rsub__(self, o): return Tensor(self._v(o) - self.a)
    def __mul__(self, o): return Tensor(self.a * self._v(o))
    def __rmul__(self, o): return Tensor(self._v(o) * self.a)
    def __truediv__(self, o): return Tensor(self.a / self._v(o))
    def __neg__(self): return Tensor(-self.a)


def _t(x):
    return x if isinstance(x, Tensor) else Tensor(x)


def install_stand_in():
    K = types.ModuleType("keras.backend")
    K.round = lambda x: Tensor(np.rint(_t(x).a))
    K.clip = lambda x, lo, hi: Tensor(np.clip(_t(x).a, F32(lo), F32(hi)))
    K.stop_gradient = lambda x: x
    keras = types.ModuleType("keras")
    keras.backend = K
    tf = types.ModuleType("tensorflow")
    tf.nn = types.SimpleNamespace(relu=lambda x: Tensor(np.maximum(_t(x).a, F32(0))))
    tf.convert_to_tensor = lambda v: v
    tf.cast = lambda v, dtype: Tensor(np.asarray(v.a if isinstance(v, Tensor) else v).astype(dtype))
    for name, mod in {"keras": keras, "keras.backend": K, "tensorflow": tf}.items():
        assert name not in sys.modules, "a real %s is importable: use it instead of the stand-in" % name
        sys.modules[name] = mod


def around(v):
    """v (float64 points) rounded to float32, with both float32 neighbours of each."""
    c = np.asarray(v, dtype=np.float64).astype(F32)
    return np.concatenate([c, np.nextafter(c, F32(-np.inf)), np.nextafter(c, F32(np.inf))]).astype(F32)


def inputs(nb):
    m = 2.0 ** (nb - 1)
    k = np.arange(-2 * m - 2, 2 * m + 2)
    ties = (k + 0.5) / m
    pts = [around(ties), around(ties - 1.0), around(10.0 * ties),
           np.array([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25], dtype=F32),
           around([1.0, -1.0, 1.0 - 1.0 / m, -10.0, 0.0])]
    return np.concatenate(pts).astype(F32)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    install_stand_in()
    sys.path.insert(0, ref)
    from layers import quantized_ops            # the reference's file, executed as it is
    # the uniform values are shared by the four widths (one incompressible array instead of four: the file stays under the
    # repository's 1 MiB limit); every x_nb<nb> is its own edge values followed by them
    uniform = np.random.default_rng(20260106).uniform(-1.5, 1.5, 100000).astype(F32)
    out = {"x_uniform": uniform}
    for nb in NBS:
        out["x_edges_nb%d" % nb] = inputs(nb)
        x = np.concatenate([out["x_edges_nb%d" % nb], uniform])
        out["relu_nb%d" % nb] = quantized_ops.quantized_relu(Tensor(x), nb=nb).a
        out["leaky_nb%d" % nb] = quantized_ops.quantized_leakyrelu(Tensor(x), nb=nb).a
    path = os.path.join(HERE, "ref_qrelu.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
