"""quantized_relu / quantized_leakyrelu without a GPU: the arithmetic contracts against the reference's own vectors, and
the Python surface (ABI constants, the ops' arguments, the spec builders' keyword, the checkpoint name mapping)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi, engine, nets
from oracle import qnn_oracle as O
import qrelu_cases as Q

quantized_ops = engine.quantized_ops          # (the module the package itself uses)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.mark.parametrize("nb", Q.NBS)
def test_the_contracts_equal_the_reference_vectors_bit_for_bit(nb):
    x, relu, leaky = Q.fixture(nb)
    assert x.size > 100000 and relu.shape == leaky.shape == x.shape
    assert Q.same_bits(Q.quantized_relu(x, nb), relu)
    assert Q.same_bits(Q.quantized_leakyrelu(x, nb), leaky)
    assert Q.same_bits(O.quantized_relu_unused(x, nb), relu)
    # the strip kernels' max(v, 0.1f * v) is the contract's select for every sign of v
    assert Q.same_bits(Q.quantized_leakyrelu_max_form(x, nb), leaky)
    neg, pos = x[x < 0], x[x >= 0]
    assert np.all((Q.ALPHA * neg).astype(F32) >= neg) and np.all((Q.ALPHA * pos).astype(F32) <= pos)


@pytest.mark.parametrize("nb", Q.NBS)
def test_the_vectors_hold_the_points_the_contracts_turn_on(nb):
    x, relu, leaky = Q.fixture(nb)
    m = 2.0 ** (nb - 1)
    have = set(x.view(np.int32).tolist())
    def has(v):
        return int(np.asarray(v, dtype=F32).view(np.int32)) in have
    for k in range(int(-m) - 1, int(m) + 1):
        for t in ((k + 0.5) / m, (k + 0.5) / m - 1.0):
            c = F32(t)
            assert has(c) and has(np.nextafter(c, F32(-np.inf))) and has(np.nextafter(c, F32(np.inf))), (nb, k, t)
    for v in (0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25):
        assert has(v), v
    for e in (1.0, -1.0, 1.0 - 1.0 / m):
        assert has(np.nextafter(F32(e), F32(-np.inf))) and has(np.nextafter(F32(e), F32(np.inf))), e
    assert x.min() < -1.49 and x.max() > 1.49
    # both grids are reached end to end
    assert set(np.unique(relu * F32(m)).tolist()) == set(range(0, int(m)))
    assert set(np.unique(leaky * F32(m)).tolist()) >= set(range(0, int(m))) and leaky.min() < 0 if nb > 2 else True
    # quantized_relu is not quantized_tanh clamped at 0: v + 1 discards low bits of v
    tiny = np.array([2.0 ** -25, -2.0 ** -25], dtype=F32)
    assert np.array_equal(Q.quantized_relu(tiny, nb), np.zeros(2, F32))
    assert np.count_nonzero(np.clip(O.quantized_tanh(x, nb), 0, None) != relu) > 0


def test_abi_constants_and_the_extension_header():
    hdr = open(os.path.join(ROOT, "include", "qnn_abi.h")).read()
    assert re.search(r"#define QNN_FN_QUANTIZED_RELU\s+6\b", hdr) and re.search(r"#define QNN_FN_QUANTIZED_LEAKYRELU\s+7\b", hdr)
    assert (_abi.FN_QUANTIZED_RELU, _abi.FN_QUANTIZED_LEAKYRELU) == (6, 7)
    assert _abi.QUANT_FNS == (_abi.FN_QUANTIZED_TANH, 6, 7)
    ext = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qnn_abi_qact.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(qnn_[a-z0-9_]+)\s*\(", ext))) == sorted(_abi.EXPORTS_QACT) == ["qnn_quantized_act_f32"]
    assert not set(_abi.EXPORTS_QACT) & set(_abi.EXPORTS) and len(_abi.EXPORTS) == 29
    lib = ctypes.CDLL(_abi.lib_path())
    assert hasattr(lib, "qnn_quantized_act_f32")
    lib = _abi.load()
    assert lib.qnn_version() == 4
    # argument checks come before any device call
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    assert lib.qnn_quantized_act_f32(buf, buf, 4, _abi.FN_BINARY_TANH, 4, None) == -1
    assert b"not a quantised activation" in lib.qnn_last_error()
    assert lib.qnn_quantized_act_f32(buf, buf, 4, _abi.FN_QUANTIZED_RELU, 25, None) == -1
    assert lib.qnn_quantized_act_f32(None, buf, 4, _abi.FN_QUANTIZED_RELU, 4, None) == -1
    assert lib.qnn_quantized_act_f32(buf, buf, 0, _abi.FN_QUANTIZED_LEAKYRELU, 4, None) == 0      # nothing to launch
    # BIN storage is refused for the two functions, as for quantized_tanh
    for fn in (_abi.FN_QUANTIZED_RELU, _abi.FN_QUANTIZED_LEAKYRELU):
        assert lib.qnn_pack_f32(buf, buf, 1, 8, fn, 2, _abi.STORE_BIN, None) == -1
        assert lib.qnn_pack_f32(buf, buf, 1, 8, fn, 5, _abi.STORE_I4, None) == -1                  # act_bits <= store
        assert lib.qnn_pack_f32(buf, buf, 0, 8, fn, 4, _abi.STORE_I4, None) == 0


def test_python_surface():
    assert qnn_amd.quantized_relu is quantized_ops.quantized_relu
    assert qnn_amd.quantized_leakyrelu is quantized_ops.quantized_leakyrelu
    x = torch.zeros(4, 4)
    for bad in (0.3, 0.0, 0.1000001, 1):
        with pytest.raises(ValueError):
            quantized_ops.quantized_leakyrelu(x, 4, alpha=bad)
    for fn in (quantized_ops.quantized_relu, quantized_ops.quantized_leakyrelu):
        with pytest.raises(_abi.QnnError):          # the default alpha passes the check; there is no CPU path behind it
            fn(x, 4)
    with pytest.raises(_abi.QnnError):
        quantized_ops.quantized_leakyrelu(x, 4, alpha=np.float32(0.1))
    # the layer classes take the functions as activation=, and fuse them on load as the preceding activation
    layer = qnn_amd.QuantizedConv2D(8, kernel_size=3, padding="same", nb=4, H=1, activation=qnn_amd.quantized_relu, device="cpu")
    assert layer.activation is qnn_amd.quantized_relu
    layer.build((None, 4, 4, 8))
    for dom, fn in ((("quantized_relu", 4), _abi.FN_QUANTIZED_RELU), (("quantized_leakyrelu", 3), _abi.FN_QUANTIZED_LEAKYRELU),
                    (("quantized_tanh", 4), _abi.FN_QUANTIZED_TANH)):
        layer.input_domain = dom
        assert layer._plan() == (_abi.STORE_I4, dom[1], fn, dom[1])
    # the engines' one fn mapping, and the grid a layer may assume behind the activation
    assert engine._act_code({"op": "act", "fn": "quantized_relu", "nb": 4}) == (_abi.FN_QUANTIZED_RELU, 4)
    assert engine._act_code({"op": "act", "fn": "quantized_leakyrelu", "nb": 8}) == (_abi.FN_QUANTIZED_LEAKYRELU, 8)
    assert engine._act_code({"op": "act", "fn": "quantized_relu", "nb": 16}) is None
    with pytest.raises(ValueError):
        engine._act_code({"op": "act", "fn": "quantized_leakyrelu", "nb": 4, "alpha": 0.3})
    assert engine.LayerModel._grid({"op": "act", "fn": "quantized_leakyrelu", "nb": 4}) == ("quantized", 4)


@pytest.mark.parametrize("fn", Q.FNS)
def test_spec_builders_take_the_activation(fn):
    for nt in ("full-qnn", "qbnn", "qtnn"):
        for arch in ("VGG", "RESNET"):
            cf = nets.Config(network_type=nt, wbits=4, abits=3, architecture=arch, nres=1)
            spec = nets.build_spec(cf, 3, quantized_activation=fn)
            acts = [op for op in spec if op["op"] == "act"]
            assert acts and all(a["fn"] == fn and a["nb"] == 3 for a in acts), (nt, arch)
            base = nets.build_spec(cf, 3)
            assert [op["op"] for op in base] == [op["op"] for op in spec]
            assert all(a["fn"] == "quantized_tanh" for a in base if a["op"] == "act")
            assert all(np.array_equal(a["kernel"], b["kernel"]) for a, b in zip(base, spec) if a["op"] in ("conv", "dense"))
    # the other network types have no quantised activation to replace
    for nt in ("qnn", "full-bnn", "float"):
        spec = nets.build_spec(nets.Config(network_type=nt), 3, quantized_activation=fn)
        assert all(a["fn"] != fn for a in spec if a["op"] == "act")
    with pytest.raises(ValueError):
        nets.build_spec(nets.Config(), 3, quantized_activation="quantized_maxrelu")
    # a fused chain and a residual plan are made of it: no fold is ever asked for
    rcf = nets.Config(network_type="full-qnn", wbits=4, abits=4, architecture="RESNET", nres=1, dim=16)
    m = engine.ResidualFusedModel(nets.build_spec(rcf, 2, quantized_activation=fn), device="cpu")
    acts = [n for n, i in m.prod.items() if m.spec[i]["op"] == "act"]
    assert {m._act_out_store(n, 4) for n in acts} == {_abi.STORE_I4}
    assert all(m._plan(n)[3] is None for n in acts)             # and no in-launch projection is planned either way


def test_a_checkpoints_quantized_relu_stays_quantized_tanh():
    """Activation('quantized_relu') in a checkpoint is the reference's shadowing lambda (model_factory.py:19-20)."""
    spec = nets.spec_from_keras_npz(os.path.join(ROOT, "tests", "golden", "resnet3_full_44.npz"), 4, 4)
    acts = [op for op in spec if op["op"] == "act"]
    assert len(acts) >= 10 and all(a["fn"] == "quantized_tanh" and a["nb"] == 4 for a in acts)
