"""Channel concatenation without a GPU: the extension header and its argument checks (no device is touched before them),
the numpy reference of concat_cases.py against the suite's restatement of the packed layout, the layer class, the
checkpoint importer, the spec graph's reading of the op and the refusal of the engines that do not express it."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi, engine, nets

import concat_cases as C
import tail_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
EINVAL, EUNSUPPORTED = -1, -2
ENTRY = _abi.EXPORTS_CONCAT[0]           # read at import: without the entry, the op and the class nothing below means anything
LAYER = qnn_amd.Concatenate


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_the_extension_header_and_the_exports():
    hdr = open(os.path.join(ROOT, "include", "qnn_abi_concat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(qnn_[a-z0-9_]+)\s*\(", code))) == sorted(_abi.EXPORTS_CONCAT)
    assert _abi.EXPORTS_CONCAT == ["qnn_concat_forward"]
    assert re.search(r"#define QNN_CONCAT_MAX\s+8\b", hdr) and _abi.CONCAT_MAX == 8 == C.MAX_INPUTS
    body = re.search(r"typedef struct qnn_concat \{([^{}]*)\} qnn_concat_t;", code).group(1)
    fields = [re.sub(r"\[.*\]", "", d.split()[-1].lstrip("*")) for d in body.split(";") if d.strip()]
    assert fields == [n for n, _ in _abi.Concat._fields_] == ["n", "channels", "x"]
    assert ctypes.sizeof(_abi.Concat) == 4 + 4 * 8 + 4 + 8 * 8          # n, channels, padding to the pointers, x
    others = _abi.EXPORTS + _abi.EXPORTS_QACT + _abi.EXPORTS_DILATION + _abi.EXPORTS_MAXACT + _abi.EXPORTS_POOL + \
        _abi.EXPORTS_SCALED
    assert not set(_abi.EXPORTS_CONCAT) & set(others)
    assert len(_abi.EXPORTS) == 29                   # qnn_abi.h's own list is what it was
    lib = ctypes.CDLL(_abi.lib_path())
    assert hasattr(lib, "qnn_concat_forward")
    assert _abi.load().qnn_version() == 4


def _desc(channels, ptrs=None):
    d = _abi.Concat()
    d.n = len(channels)
    for i, c in enumerate(channels[:8]):
        d.channels[i] = c
        d.x[i] = ((1 << 40) + (i << 32)) if ptrs is None else ptrs[i]
    return d


def test_forward_refuses_bad_arguments_before_any_device_call():
    """No GPU here: every answer below is given before the first HIP call.  The pointers are never read."""
    lib = _abi.load()
    y = ctypes.c_void_p(1 << 50)
    F, B, T2, I4, I8 = _abi.STORE_F32, _abi.STORE_BIN, _abi.STORE_T2, _abi.STORE_I4, _abi.STORE_I8

    def fwd(channels=(3, 5), store=I4, bits=4, pixels=7, yp=y, ptrs=None, n=None, d="make"):
        if d == "make":
            d = _desc(list(channels), ptrs)
            if n is not None:
                d.n = n
        rc = lib.qnn_concat_forward(ctypes.byref(d) if d is not None else None, store, bits, pixels, yp, None)
        if rc != 0:
            assert b"qnn_concat_forward" in lib.qnn_last_error(), lib.qnn_last_error()      # every message names the entry
        return rc

    assert fwd(d=None) == EINVAL                                               # null descriptor
    assert fwd(n=0) == EINVAL and fwd(n=9) == EINVAL and fwd(n=-1) == EINVAL   # n in 1 .. QNN_CONCAT_MAX
    assert fwd(channels=(3, 0)) == EINVAL and fwd(channels=(-2, 5)) == EINVAL and fwd(channels=(0,)) == EINVAL
    for store in (3, 5, _abi.STORE_U8, _abi.STORE_F32_IMAGE, _abi.STORE_F32_UNIT, -1):
        assert fwd(store=store) == EINVAL, store
    assert fwd(store=I4, bits=5) == EINVAL and fwd(store=I4, bits=0) == EINVAL and fwd(store=I8, bits=9) == EINVAL
    assert fwd(yp=None) == EINVAL and fwd(ptrs=[1 << 40, 0]) == EINVAL         # null pointers
    assert b"null" in lib.qnn_last_error()
    # y overlapping an input: the same address, inside it, and an input that begins inside y
    assert fwd(yp=ctypes.c_void_p(1 << 40)) == EINVAL and b"overlap" in lib.qnn_last_error()
    assert fwd(ptrs=[1 << 40, (1 << 50) + 4]) == EINVAL and b"overlap" in lib.qnn_last_error()
    assert fwd(channels=(8, 8), ptrs=[(1 << 50) - 4 * 7 + 4, 1 << 40]) == EINVAL
    # pixels x output words (channels for float32) >= 2^31
    assert fwd(channels=(8, 8), pixels=1 << 30) == EUNSUPPORTED
    assert fwd(channels=(1, 1), store=F, pixels=1 << 30) == EUNSUPPORTED
    assert fwd(channels=(32, 32), store=T2, pixels=1 << 29) == EUNSUPPORTED
    assert fwd(channels=(1 << 30, 1 << 30), store=F, pixels=1) == EUNSUPPORTED
    assert fwd(channels=(3, 5), store=B, pixels=(1 << 31) + 5) == EUNSUPPORTED
    # no pixels: fine, nothing is launched and the pointers may be null -- but only with valid arguments
    null = _desc([3, 5], [0, 0])
    for store, bits in ((F, 0), (B, 1), (T2, 1), (I4, 4), (I4, 2), (I8, 8)):
        assert fwd(store=store, bits=bits, pixels=0) == 0
        assert fwd(store=store, bits=bits, pixels=0, yp=None, d=null) == 0
    assert fwd(channels=(5,), pixels=0) == 0 and fwd(channels=(1,) * 8, pixels=0) == 0
    assert fwd(pixels=0, bits=7) == EINVAL and fwd(pixels=0, store=3) == EINVAL and fwd(pixels=0, n=0) == EINVAL
    assert fwd(pixels=0, channels=(3, 0)) == EINVAL


def test_the_binding_refuses_before_the_library():
    a, b = torch.zeros(7, 3), torch.zeros(7, 5)
    with pytest.raises(_abi.QnnError, match="no CPU path"):
        _abi.concat([a, b], [3, 5], _abi.STORE_F32, 0, 7)                      # CPU tensors
    with pytest.raises(_abi.QnnError, match="contiguous int32 CUDA"):
        _abi.concat([a.int(), b.int()], [3, 5], _abi.STORE_I4, 4, 7)
    with pytest.raises(_abi.QnnError, match="9 inputs"):
        _abi.concat([a] * 9, [3] * 9, _abi.STORE_F32, 0, 7)
    with pytest.raises(_abi.QnnError, match="0 inputs"):
        _abi.concat([], [], _abi.STORE_F32, 0, 7)
    with pytest.raises(_abi.QnnError, match="store"):
        _abi.concat([a, b], [3, 5], _abi.STORE_U8, 0, 7)
    with pytest.raises(_abi.QnnError, match="channels"):
        _abi.concat([a, b], [3, 0], _abi.STORE_F32, 0, 7)
    with pytest.raises(ValueError):
        _abi.concat([a, b], [3], _abi.STORE_F32, 0, 7)


# ---- the reference ------------------------------------------------------------------------------------------------------
def test_the_case_list_is_the_issues():
    assert C.LISTS["bin"] == [[3, 5], [32, 32], [31, 1, 33], [3] * 8, [128, 256], [64, 32]]
    assert C.LISTS["i4"] == [[3, 5], [8, 8], [7, 9, 16], [12, 24, 36], [32, 64]]
    assert C.LISTS["i8"] == [[1, 2, 5], [4, 4], [3, 64], [16, 48]]
    assert C.LISTS["t2"] == [[3, 5], [32, 31]] and C.LISTS["f32"] == [[3, 5], [4, 4], [1] * 8]
    assert C.PIXELS == (1, 7, 280) and 280 % 256 != 0
    for kind, bits in C.BITS.items():
        assert bits[0] == {"bin": 1, "t2": 1, "i4": 4, "i8": 8, "f32": 0}[kind]
        assert kind not in ("i4", "i8") or bits[1] < bits[0]
    # every form of the kernel is reached, and the lists the issue calls aligned / whole-word are
    seen = {(k, C.form(k, ch)) for k, ls in C.LISTS.items() for ch in ls}
    for kind in ("bin", "i4", "i8"):
        assert {(kind, "words4"), (kind, "words1"), (kind, "funnel")} <= seen, kind
        for ch in C.ALIGNED[kind]:
            assert C.form(kind, ch) == "words4" and C.form(kind, ch, aligned16=False) == "words1"
        for ch in C.WORD[kind]:
            assert C.form(kind, ch) == "words1"
    assert {("t2", "funnel"), ("f32", "words4"), ("f32", "words1")} <= seen
    assert C.form("bin", [3] * 8) == "funnel" and 8 * 3 < 32            # eight inputs meet in one word


@pytest.mark.parametrize("kind", ["bin", "t2", "i4", "i8"])
def test_the_reference_is_pack_of_the_concatenated_values(kind):
    store = C.STORE[kind]
    for channels in C.LISTS[kind]:
        for bits in C.BITS[kind]:
            ks = [C.codes(kind, bits, 7, c, i) for i, c in enumerate(channels)]
            ws = [C.encode(k, kind) for k in ks]
            for k, w, c in zip(ks, ws, channels):
                np.testing.assert_array_equal(w, T.pack_words(k, store))       # the layout, against the suite's restatement
                assert w.shape == (7, C.words(kind, c)) == (7, T.words(store, c))
                np.testing.assert_array_equal(C.decode(w, kind, c), k)
                assert not np.any(w & C.spare(kind, c))
            want = T.pack_words(np.concatenate(ks, axis=-1), store)
            np.testing.assert_array_equal(C.concat_ref(ws, channels, kind), want)
            # the inputs' spare bits take no part
            dirty = [w | C.spare(kind, c) for w, c in zip(ws, channels)]
            assert any(np.any(d != w) for d, w in zip(dirty, ws)) == any(C.spare(kind, c).any() for c in channels)
            np.testing.assert_array_equal(C.concat_ref(dirty, channels, kind), want)
            assert not np.any(want[:, -2:] & C.spare(kind, sum(channels))[-2:])


def test_spare_bits():
    assert C.spare("bin", 3).tolist() == [0xFFFFFFF8] and C.spare("bin", 32).tolist() == [0]
    assert C.spare("i4", 9).tolist() == [0, 0xFFFFFFF0] and C.spare("i8", 5).tolist() == [0, 0xFFFFFF00]
    assert C.spare("t2", 33).tolist() == [0, 0, 0xFFFFFFFE, 0xFFFFFFFE]


# ---- the layer class ----------------------------------------------------------------------------------------------------
def test_layer_class():
    assert "Concatenate" in qnn_amd.__all__
    l = qnn_amd.Concatenate()
    assert l.axis == -1 and l.get_config() == {"name": "concatenate", "trainable": True, "axis": -1}
    l = qnn_amd.Concatenate(axis=3, name="cat")
    cfg = l.get_config()
    assert set(cfg) == {"name", "trainable", "axis"} and cfg["axis"] == 3 and cfg["name"] == "cat"
    assert qnn_amd.Concatenate.from_config(cfg).get_config() == cfg
    assert l.compute_output_shape([(None, 8, 8, 12), (None, 8, 8, 24)]) == (None, 8, 8, 36)
    assert qnn_amd.Concatenate(axis=1).compute_output_shape([(4, 10), (4, 3), (4, 1)]) == (4, 14)
    a, b = torch.zeros(2, 4, 4, 3), torch.zeros(2, 4, 4, 5)
    for axis in (0, 1, 2, -2):
        with pytest.raises(_abi.QnnError, match="axis=%d" % axis):
            qnn_amd.Concatenate(axis=axis)([a, b])
    for axis in (0, 2, 3):
        with pytest.raises(_abi.QnnError, match="axis=%d" % axis):
            qnn_amd.Concatenate(axis=axis)([torch.zeros(2, 3), torch.zeros(2, 5)])
    for bad in ([a], [], a):
        with pytest.raises(ValueError, match="should be called on a list of at least 2 inputs"):
            qnn_amd.Concatenate()(bad)
    for other in (torch.zeros(2, 4, 5, 5), torch.zeros(3, 4, 4, 5), torch.zeros(2, 16)):
        with pytest.raises(ValueError, match="requires inputs with matching shapes except for the concat axis"):
            qnn_amd.Concatenate()([a, other])
    for axis in (-1, 3):
        with pytest.raises(_abi.QnnError, match="no CPU path"):
            qnn_amd.Concatenate(axis=axis)([a, b])                             # CPU tensors: there is no CPU path


# ---- the importer ---------------------------------------------------------------------------------------------------------
def _npz(tmp_path, axis):
    layer = lambda cls, name, inbound, **c: {"class_name": cls, "name": name, "config": dict(c, name=name),      # noqa: E731
                                             "inbound_nodes": [[[i, 0, 0, {}] for i in inbound]] if inbound else []}
    pool = dict(pool_size=[3, 3], strides=[2, 2], padding="same", data_format="channels_last")
    cfg = {"class_name": "Model", "config": {"layers": [
        layer("InputLayer", "in", []),
        layer("MaxPooling2D", "p", ["in"], **pool),
        layer("AveragePooling2D", "q", ["in"], **pool),
        layer("Concatenate", "cat", ["p", "q"], axis=axis, trainable=True),
        layer("Concatenate", "cat2", ["in", "in", "cat"], axis=axis, trainable=True),
        layer("Flatten", "f", ["cat2"])]}}
    path = tmp_path / "m.npz"
    np.savez(path, model_config_json=np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8))
    return str(path)


def test_importer_maps_concatenate(tmp_path):
    for axis in (-1, 3):
        spec = nets.spec_from_keras_npz(_npz(tmp_path, axis))
        assert spec[2] == {"op": "concat", "srcs": ["p", "q"], "dst": "cat"}
        assert spec[3] == {"op": "concat", "srcs": ["input", "input", "cat"], "dst": "cat2"}       # the model input's alias
        assert spec[4] == {"op": "flatten", "src": "cat2", "dst": "f"}
    for axis in (0, 1, 2, -2):
        with pytest.raises(ValueError, match="axis=%d" % axis):
            nets.spec_from_keras_npz(_npz(tmp_path, axis))


# ---- the engines' reading of the op ---------------------------------------------------------------------------------------
def test_spec_graph_lists_every_source_of_a_concat():
    net = C.SPECS["densenet"][0]
    spec = net.spec
    g = _graph(spec)
    assert g.srcs == C.sources(spec)
    for i, op in enumerate(spec):
        if op["op"] == "concat":
            assert g.srcs[i] == op["srcs"] and len(op["srcs"]) == 2
            for s in op["srcs"]:
                assert i in g.cons[s] and s in g.prod           # consumer of each source, each source has a producer
    # the stem is read by the first block's conv and by the first concat; a concat by the next conv and the next concat
    assert [spec[i]["op"] for i in g.cons["stem"]] == ["conv", "concat"]
    assert [spec[i]["op"] for i in g.cons["dense0"]] == ["conv", "concat"]
    assert [spec[i]["op"] for i in g.cons["dense2"]] == ["avgpool"]
    three = [{"op": "concat", "srcs": ["input", "input", "input"], "dst": "c"}]
    assert _graph(three).srcs == [["input"] * 3] and _graph(three).cons == {"input": [0, 0, 0]}


def _graph(spec):
    return engine._SpecGraph(spec, "cpu")                    # the reading of the spec alone: the BN constants stay on the host


@pytest.mark.parametrize("name", list(C.SPECS))
def test_the_other_engines_refuse_a_concat_by_name(name):
    spec = C.SPECS[name][0].spec
    assert any(op["op"] == "concat" for op in spec)
    for cls in (engine.FusedModel, engine.ResidualFusedModel, engine.LayerModel):
        with pytest.raises(_abi.NotFusable, match="concat"):
            cls(spec)


def test_the_residual_planner_takes_a_concat_for_a_float32_consumer():
    spec = C.SPECS["virtual"][0].spec
    m = engine.ResidualFusedModel.__new__(engine.ResidualFusedModel)
    g = _graph(spec)
    m.spec, m.names, m.prod, m.srcs, m.cons = spec, g.names, g.prod, g.srcs, g.cons
    assert m._act_out_store("a0", 4) == _abi.STORE_I4           # read by two convs
    assert m._act_out_store("a1", 4) is None and m._act_out_store("a2", 4) is None      # read by the concat
    assert [u["op"] for u in m._users_through_pools("a1")] == ["concat"]


def test_the_spec_reference_and_the_guard():
    for name, (net, _) in C.SPECS.items():
        x = net.images()
        assert C.guard(net.spec, x) is None, name
        env = C.reference(net.spec, x, return_all=True)
        for i, op in enumerate(net.spec):
            if op["op"] == "concat":
                y = env[op["dst"]]
                assert y.shape[-1] == sum(env[s].shape[-1] for s in op["srcs"]) and y.shape[1:] == net.shape[op["dst"]]
                at = 0
                for s in op["srcs"]:
                    np.testing.assert_array_equal(y[..., at:at + env[s].shape[-1]], env[s])
                    at += env[s].shape[-1]
        assert env[C.S.names_of(net.spec)[-1]].shape == (C.S.N, 10)
    d = C.SPECS["densenet"][0]
    assert [d.shape["dense%d" % b][-1] for b in range(3)] == [36, 48, 60] and d.hw == (8, 8)
    # a spec without the op: the runner is spec_graph_cases' own
    plain = C.S.HAND[0]
    np.testing.assert_array_equal(C.reference(plain["spec"], plain["x"]), C.S.reference(plain["spec"], plain["x"]))
