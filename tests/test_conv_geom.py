"""The output-size rule of the convolutions (csrc/qnn_conv_geom.h: qnn_same_pad) against three independent statements of
it.  No GPU: the header is plain C++, compiled here into a stand-alone program with the address and undefined-behaviour
sanitizers.

  (a) a brute-force count written below: VALID = the window starts 0, s, 2s, ... whose window lies wholly inside the
      image; SAME = ceil(in / s) with before = max((out - 1) * s + k - in, 0) // 2 (the TensorFlow documentation);
  (b) oracle.same_padding (SAME only: the oracle has no function of its own for VALID);
  (c) _abi.out_hw, which sizes every output tensor the binding allocates.

The rule this replaced computed VALID as (in - k) / s + 1 with C's truncating division: 1 instead of "no output" at the
PARENT_WRONG = 32 grid points with 0 < k - in < s (in=2 k=3 s=2, in=1 k=2 s=2, in=4 k=5 s=2, ...), so the library ran
one truncated window into a buffer the binding had sized for nothing.  test_an_image_smaller_than_the_window_has_no_output
fails with that rule at exactly those points and nowhere else; its other in < k points gave 0 or a negative size, which
the `> 0` check of conv_describe refused already.  test_an_empty_axis_is_zero pins the form both sides now share."""
import itertools
import os
import shutil
import subprocess

import pytest

import qnn_amd                                   # noqa: F401  (the package alias of conftest.py)
from qnn_amd import _abi
from oracle import qnn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quantizedneuralnetworks-keras-tensorflow_amd", "csrc")

MAIN = r"""
#include <stdio.h>
#include "qnn_conv_geom.h"
int main() {
    int in, k, s, same;
    while (scanf("%d %d %d %d", &in, &k, &s, &same) == 4) {
        int out = -12345, before = -12345;
        qnn_same_pad(in, k, s, same, &out, &before);
        printf("%d %d\n", out, before);
    }
    return 0;
}
"""

GRID = list(itertools.product(range(1, 41), range(1, 8), range(1, 5), (0, 1)))      # (in, k, s, same)
PARENT_WRONG = 32


def brute(size, k, s, same):
    """(out, before) by counting."""
    if same:
        out = -(-size // s)
        return out, max((out - 1) * s + k - size, 0) // 2
    return sum(1 for start in range(0, size, s) if start + k <= size), 0


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("conv_geom")
    src, exe = d / "geom_main.cpp", d / "geom_main"
    src.write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    text = "".join("%d %d %d %d\n" % c for c in GRID)
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
    out = [tuple(int(v) for v in ln.split()) for ln in out if ln]
    assert len(out) == len(GRID)
    return dict(zip(GRID, out))


def test_the_truncating_quotient_is_wrong_at_32_points():
    """The count the module docstring states, from the old formula itself (Python's int() truncates as C does)."""
    wrong = [(n, k, s) for n, k, s, same in GRID
             if not same and (int((n - k) / s) + 1 > 0) != (brute(n, k, s, 0)[0] > 0)]
    assert len(wrong) == PARENT_WRONG
    assert all(0 < k - n < s for n, k, s in wrong)
    assert {(2, 3, 2), (1, 2, 2), (1, 3, 3), (2, 3, 3), (4, 5, 2)} <= set(wrong)
    # where the image holds the window the quotient was right
    assert all(int((n - k) / s) + 1 == brute(n, k, s, 0)[0] for n, k, s, same in GRID if not same and n >= k)


def test_an_image_smaller_than_the_window_has_no_output(rule):
    """C header, oracle and binding against the count: the same axes are empty, and every other axis has the same size
    and leading padding."""
    for case in GRID:
        n, k, s, same = case
        want, want_before = brute(n, k, s, same)
        got, before = rule[case]
        assert (got > 0) == (want > 0), ("qnn_same_pad", case, got, want)
        assert (_abi.out_hw(n, k, s, bool(same)) > 0) == (want > 0), ("out_hw", case)
        if want > 0:
            assert (got, before) == (want, want_before), ("qnn_same_pad", case, (got, before), (want, want_before))
            assert _abi.out_hw(n, k, s, bool(same)) == want, ("out_hw", case)
        if same:
            o_out, o_before, o_after = O.same_padding(n, k, s)
            assert (o_out, o_before) == (want, want_before), ("oracle", case)
            assert o_before + o_after == max((want - 1) * s + k - n, 0) and 0 <= o_after - o_before <= 1, ("oracle", case)
            assert want >= 1                         # SAME never yields an empty axis


def test_an_empty_axis_is_zero(rule):
    """in < k under VALID is exactly 0 on both sides (never negative), so Python and C cannot disagree about it."""
    empty = [c for c in GRID if not c[3] and c[0] < c[1]]
    assert len(empty) == 4 * sum(k - 1 for k in range(1, 8))
    for case in empty:
        n, k, s, _ = case
        assert brute(n, k, s, 0) == (0, 0)
        assert rule[case] == (0, 0), case
        assert _abi.out_hw(n, k, s, False) == 0, case


def test_the_binding_refuses_an_empty_output_before_any_library_call():
    """_abi.conv2d and its siblings size their output through _stored_hw: an empty axis, before or after pooling, is a
    QnnError raised before the library is touched (this test has no GPU and no handle)."""
    class W:                                         # what _stored_hw reads of a Weights
        def __init__(self, kh, kw, stride, same):
            self.shape, self.stride, self.same_pad = (kh, kw, 4, 4), stride, same
    for H, Wd, kh, kw, s in ((2, 9, 3, 3, 2), (9, 2, 3, 3, 2), (1, 5, 2, 2, 2), (5, 1, 3, 3, 3), (4, 9, 5, 5, 2), (1, 1, 7, 7, 1)):
        with pytest.raises(_abi.QnnError, match="empty output"):
            _abi._stored_hw("conv2d", W(kh, kw, s, False), H, Wd, 1)
    with pytest.raises(_abi.QnnError, match="empty output"):
        _abi._stored_hw("conv2d", W(3, 3, 1, False), 3, 9, 2)          # 1 x 7 conv map, pooled by 2
    with pytest.raises(_abi.QnnError, match="empty output"):
        _abi._stored_hw("conv2d", W(1, 1, 3, True), 3, 3, 2)           # SAME stride 3: 1 x 1, pooled by 2
    assert _abi._stored_hw("conv2d", W(3, 3, 2, False), 3, 9, 1) == (1, 4)
    assert _abi._stored_hw("conv2d", W(2, 3, 1, True), 5, 7, 2) == (2, 3)
