#!/usr/bin/env python3
"""Reference vectors for quantized_maxrelu and quantized_leakymaxrelu: tests/golden/ref_maxrelu.npz.

    python tests/golden/make_fixtures_maxrelu.py [/root/reference]

For the build container only (the reference checkout is not part of this repository, and no test runs this file).  It
EXECUTES the reference's own layers/quantized_ops.py, imported from where it lies, on float32 numpy arrays, with the
eager float32 stand-in of make_fixtures_qrelu.py plus the four operations only these two functions call: tf.reduce_max,
tf.log, tf.ceil and tf.pow, each one numpy float32 operation.  The op sequence, the constants and their order are the
reference's; nothing of its text is copied here.

Group 1, compared bit for bit by tests/test_maxrelu_cpu.py -- nb in {2, 3, 4, 8}, maximum M = mant * 2^k with mant in
{1.0625, 1.5, 1.9375} and k in {-3, 0, 1, 5} (far from a power of two: ceil(log(M) / log(2)) is k + 1 whatever the log's
last bits), so P = 2^(k+1), step = P / m, m = 2^(nb-1).  Inputs of a case (maxrelu_cases.edge_inputs, every value <= M):
  M itself;  every tie (j + 1/2) step, j = -m-1 .. m, and the leaky side's ties 10 (j + 1/2) step, j = -m-1 .. -1, each
  with both float32 neighbours;  +-0;  the clip edges (m - 1) step, -m step, -10 m step and 0 with both neighbours;
  2000 uniform values in [-1.5 M, M].
Arrays: g1_x_nb<nb>_<case> (edges), g1_u_<case> (the uniform values, shared by the four widths of a maximum),
g1_max_nb<nb>_<case>, g1_leaky_nb<nb>_<case> (alpha = the reference's default 0.1) -- outputs as returned, float32;
<case> = index into maxrelu_cases.MAXIMA.

Group 2, RECORDED, not asserted equal -- M exactly 2^k and 2^k + 1 .. 16 ulp for k in {-15, 0, 13}: here the quotient
of the two float32 logarithms may fall on either side of the integer, so the stand-in's scale (numpy's float32 log on
the machine that ran this file) may be twice or half the exact one.  Arrays: g2_x_<i> (128 values <= M, M first),
g2_max_nb<nb>_<i>, g2_leaky_nb<nb>_<i>, i = index into maxrelu_cases.AMBIGUOUS.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_fixtures_qrelu as base          # the float32 stand-in of keras.backend / tensorflow
import maxrelu_cases as C                   # the case list and the input points (no arithmetic of the ops)

Tensor = base.Tensor


def extend_stand_in():
    tf = sys.modules["tensorflow"]
    tf.reduce_max = lambda x: Tensor(np.max(base._t(x).a))
    tf.log = lambda x: Tensor(np.log(base._t(x).a))
    tf.ceil = lambda x: Tensor(np.ceil(base._t(x).a))
    tf.pow = lambda b, e: Tensor(np.power(np.float32(b), base._t(e).a))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    base.install_stand_in()
    extend_stand_in()
    sys.path.insert(0, ref)
    from layers import quantized_ops            # the reference's file, executed as it is
    out = {}
    for ci, M in enumerate(C.MAXIMA):
        out["g1_u_%d" % ci] = C.uniform_inputs(M, ci)
        for nb in C.NBS:
            out["g1_x_nb%d_%d" % (nb, ci)] = C.edge_inputs(nb, M)
            x = np.concatenate([out["g1_x_nb%d_%d" % (nb, ci)], out["g1_u_%d" % ci]])
            assert x.max() == M
            out["g1_max_nb%d_%d" % (nb, ci)] = quantized_ops.quantized_maxrelu(Tensor(x), nb=nb).a
            out["g1_leaky_nb%d_%d" % (nb, ci)] = quantized_ops.quantized_leakymaxrelu(Tensor(x), nb=nb).a
    for i, M in enumerate(C.AMBIGUOUS):
        x = out["g2_x_%d" % i] = C.ambiguous_inputs(M, i)
        assert x.max() == M
        for nb in C.NBS:
            out["g2_max_nb%d_%d" % (nb, i)] = quantized_ops.quantized_maxrelu(Tensor(x), nb=nb).a
            out["g2_leaky_nb%d_%d" % (nb, i)] = quantized_ops.quantized_leakymaxrelu(Tensor(x), nb=nb).a
    path = os.path.join(HERE, "ref_maxrelu.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
