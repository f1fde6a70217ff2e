"""dilation_rate of the conv layers, host side (no GPU): the expected values of tests/test_gpu_conv_dilation.py, the
geometry rule, and the Python surface.

  * A dilated convolution is the plain convolution with the zero-stuffed kernel (conv_dilation_cases.stuff).  That claim
    is proven here on every case of the shared list against torch.nn.functional.conv2d(..., dilation=d) in float64, with
    TensorFlow's SAME padding on the effective window applied explicitly.  All tensors are dyadic: the comparison is exact.
  * csrc/qnn_conv_geom.h's qnn_same_pad_dilated is compiled into a stand-alone program (its own main, address and
    undefined-behaviour sanitizers) and compared with a brute-force count and with _abi.out_hw.
  * The three conv classes accept dilation_rate, report it, size their output with it and refuse it with strides != 1 as
    Keras does; spec_from_keras_npz keeps the key.  The constructor cases fail without the feature (QnnError before)."""
import ctypes
import itertools
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi, nets
from oracle import qnn_oracle as O
import conv_dilation_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quantizedneuralnetworks-keras-tensorflow_amd", "csrc")


@pytest.mark.parametrize("window", D.WINDOWS, ids=lambda w: "%dx%d" % w)
def test_zero_stuffed_oracle_conv_equals_torch_dilated_conv(window):
    for g in (g for g in D.geometries() if (g["kh"], g["kw"]) == window):
        x, k, _ = D.layer_values("i4", g, 3, 4)
        Ho, Wo = D.out_hw(g)
        if Ho <= 0 or Wo <= 0:
            assert g["padding"] == "valid"           # SAME always has an output
            continue
        got = O.conv2d(x, D.stuff(k, g["dh"], g["dw"]), (1, 1), g["padding"])
        xt = torch.as_tensor(x.astype(np.float64)).permute(0, 3, 1, 2)
        if g["padding"] == "same":                   # total ke - 1 per axis, the odd cell after
            pt, pl = D.same_before(g["H"], g["kh"], g["dh"]), D.same_before(g["W"], g["kw"], g["dw"])
            pb = D.effective(g["kh"], g["dh"]) - 1 - pt
            pr = D.effective(g["kw"], g["dw"]) - 1 - pl
            xt = torch.nn.functional.pad(xt, (pl, pr, pt, pb))
        wt = torch.as_tensor(k.astype(np.float64)).permute(3, 2, 0, 1)
        want = torch.nn.functional.conv2d(xt, wt, dilation=(g["dh"], g["dw"])).permute(0, 2, 3, 1).numpy()
        assert got.shape == (D.N, Ho, Wo, 4), D.geom_id(g)
        np.testing.assert_array_equal(got.astype(np.float64), want, err_msg=D.geom_id(g))


def test_out_hw_with_dilation():
    for size, k, d, same in itertools.product(range(1, 25), (1, 2, 3), range(1, 9), (False, True)):
        assert _abi.out_hw(size, k, 1, same, d) == D.out_size(size, k, d, "same" if same else "valid")
    for size, k, s, same in itertools.product(range(1, 25), (1, 2, 3), (1, 2, 3), (False, True)):
        assert _abi.out_hw(size, k, s, same) == _abi.out_hw(size, k, s, same, 1)       # the default is today's rule
    assert _abi.out_hw(4, 3, 1, False, 2) == 0 and _abi.out_hw(5, 3, 1, False, 2) == 1


MAIN = r"""
#include <stdio.h>
#include "qnn_conv_geom.h"
int main() {
    int in, k, s, d, same;
    while (scanf("%d %d %d %d %d", &in, &k, &s, &d, &same) == 5) {
        int out = -12345, before = -12345;
        qnn_same_pad_dilated(in, k, s, d, same, &out, &before);
        printf("%d %d\n", out, before);
    }
    return 0;
}
"""
GRID = list(itertools.product(range(1, 30), (1, 2, 3), (1, 2), range(1, 10), (0, 1)))      # (in, k, s, d, same)


def brute(size, k, s, d, same):
    ke = d * (k - 1) + 1
    if same:
        out = -(-size // s)
        return out, max((out - 1) * s + ke - size, 0) // 2
    return sum(1 for start in range(0, size, s) if start + ke <= size), 0


def test_the_dilated_geometry_rule_as_a_stand_alone_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src, exe = tmp_path / "geom_dil_main.cpp", tmp_path / "geom_dil_main"
    src.write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    text = "".join("%d %d %d %d %d\n" % c for c in GRID)
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
    out = [tuple(int(v) for v in ln.split()) for ln in out if ln]
    assert len(out) == len(GRID)
    for c, got in zip(GRID, out):
        size, k, s, d, same = c
        assert got == brute(*c), c
        assert got[0] == _abi.out_hw(size, k, s, bool(same), d), c
        if s == 1 and same:
            assert got == (size, D.same_before(size, k, d)), c
        if d == 1:                                   # the undilated rule is unchanged
            assert got[0] == _abi.out_hw(size, k, s, bool(same)), c


LAYERS = (lambda **kw: qnn_amd.QuantizedConv2D(8, nb=4, **kw), lambda **kw: qnn_amd.BinaryConv2D(8, **kw),
          lambda **kw: qnn_amd.TernaryConv2D(8, **kw))


@pytest.mark.parametrize("make", LAYERS, ids=("quantized", "binary", "ternary"))
def test_conv_classes_accept_dilation_rate(make):
    l = make(kernel_size=3, padding="valid", dilation_rate=2, device="cpu")
    assert l.dilation_rate == (2, 2) and l.get_config()["dilation_rate"] == (2, 2)
    assert l.compute_output_shape((None, 9, 12, 5)) == (None, 5, 8, 8)
    assert l.compute_output_shape((None, 4, 12, 5)) == (None, 0, 8, 8)         # smaller than the 5-row effective window
    l = make(kernel_size=(3, 2), padding="valid", dilation_rate=(1, 3), device="cpu")
    assert l.dilation_rate == (1, 3) and l.get_config()["dilation_rate"] == (1, 3)
    assert l.compute_output_shape((None, 9, 12, 5)) == (None, 7, 9, 8)
    l = make(kernel_size=3, padding="same", dilation_rate=(1, 3), device="cpu")
    assert l.compute_output_shape((None, 9, 12, 5)) == (None, 9, 12, 8)
    l.build((None, 9, 12, 5))
    assert tuple(l.kernel.shape) == (3, 3, 5, 8)
    with pytest.raises(ValueError, match="`strides > 1` not supported in conjunction with `dilation_rate > 1`"):
        make(kernel_size=3, strides=2, dilation_rate=2, device="cpu")
    assert make(kernel_size=3, strides=2, device="cpu").dilation_rate == (1, 1)


def test_spec_from_keras_npz_keeps_dilation_rate(tmp_path):
    def conv(name, src, **cfg):
        c = dict(name=name, use_bias=False, strides=[1, 1], padding="same", kernel_lr_multiplier=1.0)
        c.update(cfg)
        return {"class_name": "QuantizedConv2D", "name": name, "config": c, "inbound_nodes": [[[src, 0, 0, {}]]]}
    layers = [{"class_name": "InputLayer", "name": "in0", "config": {}, "inbound_nodes": []},
              conv("c0", "in0", dilation_rate=[2, 2]), conv("c1", "c0", dilation_rate=[1, 3]),
              conv("c2", "c1", dilation_rate=[1, 1]), conv("c3", "c2")]
    cfg = {"config": {"layers": layers}}
    arrays = {"model_config_json": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)}
    rng = np.random.default_rng(3)
    for n in ("c0", "c1", "c2", "c3"):
        arrays[n + "/kernel"] = (D.codes(rng, (3, 3, 4, 4), -8, 7) / 8.0).astype(np.float32)
    path = tmp_path / "tiny.npz"
    np.savez(path, **arrays)
    spec = nets.spec_from_keras_npz(str(path), wbits=4, abits=4)
    assert [op["op"] for op in spec] == ["conv"] * 4
    assert spec[0]["dilation_rate"] == (2, 2) and spec[1]["dilation_rate"] == (1, 3)
    assert "dilation_rate" not in spec[2] and "dilation_rate" not in spec[3]   # an ordinary window keeps the spec it had


def test_the_extension_header_declares_what_the_library_exports_and_the_binding_binds():
    """include/qnn_abi_dilation.h is an extension of ABI 4: its symbols are _abi.EXPORTS_DILATION, the library exports
    them, and qnn_abi.h, _abi.EXPORTS and qnn_version() stay what they were (tests/test_abi_host.py, test_abi_tail.py)."""
    def declared(name):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        return sorted(set(re.findall(r"\b(qnn_[a-z0-9_]+)\s*\(", src)))
    assert declared("qnn_abi_dilation.h") == sorted(_abi.EXPORTS_DILATION) == ["qnn_prepack_weights_dilated"]
    assert not set(_abi.EXPORTS_DILATION) & set(_abi.EXPORTS)
    assert declared("qnn_abi.h") == sorted(_abi.EXPORTS)
    lib = ctypes.CDLL(_abi.lib_path())
    for n in _abi.EXPORTS_DILATION:
        assert hasattr(lib, n), "libqnn_hip.so does not export %s" % n
    lib = _abi.load()
    assert lib.qnn_version() == 4
    assert len(lib.qnn_prepack_weights_dilated.argtypes) == len(lib.qnn_prepack_weights.argtypes) + 2
    # the argument checks come before any device call: d < 1 is QNN_EINVAL, stride 2 with d = 2 QNN_EUNSUPPORTED
    fake = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    out = ctypes.c_void_p(None)
    args = lambda stride, dh, dw: (_abi.W_QUANT, 4, 1.0, fake, 3, 3, 16, 16, None, stride, 1, dh, dw, _abi.STORE_I4, None,   # noqa: E731
                                   ctypes.byref(out))
    assert lib.qnn_prepack_weights_dilated(*args(1, 0, 1)) == -1 and b"must be >= 1" in lib.qnn_last_error()
    assert lib.qnn_prepack_weights_dilated(*args(2, 2, 2)) == _abi.QNN_EUNSUPPORTED
    assert b"together with stride 2" in lib.qnn_last_error()
    assert lib.qnn_prepack_weights_dilated(*args(1, 65, 1)) == _abi.QNN_EUNSUPPORTED and out.value is None
