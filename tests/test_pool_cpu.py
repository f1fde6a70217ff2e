"""Keras pooling without a GPU: the numpy reference of pool_cases.py against torch on float64, the output-size rule, the
extension header and its argument checks (no device is touched before them), the layer classes, the checkpoint importer
and the fused engine's refusal of a pool it cannot express."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import qnn_amd
from qnn_amd import _abi, engine, nets

import pool_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
EINVAL, EUNSUPPORTED = -1, -2


# ---- the reference -----------------------------------------------------------------------------------------------------
def _torch_pool(x, mode, size, strides, padding):
    """The same pooling from torch's own ops on float64: explicit asymmetric padding (TensorFlow's offsets) with -inf
    and max_pool2d; zero-padded window sums and the pooled ones-mask for the average (sums, counts)."""
    ph, pw = P.pair(size)
    sh, sw = (ph, pw) if strides is None else P.pair(strides)
    N, H, W, C = x.shape
    same = padding == "same"
    (Ho, pt), (Wo, pl) = P.axis(H, ph, sh, same), P.axis(W, pw, sw, same)
    pb, pr = max((Ho - 1) * sh + ph - H - pt, 0), max((Wo - 1) * sw + pw - W - pl, 0)
    t = torch.as_tensor(np.asarray(x, np.float64)).permute(0, 3, 1, 2)
    if mode == "max":
        y = TF.max_pool2d(TF.pad(t, (pl, pr, pt, pb), value=float("-inf")), (ph, pw), (sh, sw))
        return y.permute(0, 2, 3, 1).numpy()
    sums = TF.avg_pool2d(TF.pad(t, (pl, pr, pt, pb)), (ph, pw), (sh, sw), divisor_override=1)
    cnt = TF.avg_pool2d(TF.pad(torch.ones_like(t), (pl, pr, pt, pb)), (ph, pw), (sh, sw), divisor_override=1)
    return sums.permute(0, 2, 3, 1).numpy(), cnt.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("gi", range(len(P.GEOMS)))
def test_the_reference_equals_torch_on_float64(gi):
    N, H, W, size, strides, padding = P.geom(P.GEOMS[gi])
    for kind, C, bits in (("f32", 5, 0), ("i4", 9, 4), ("i8", 3, 5), ("bin", 33, 1)):
        for vset in P.VALUE_SETS:
            x = P.values(gi, kind, C, bits, vset)
            np.testing.assert_array_equal(P.expected(gi, kind, C, bits, vset, "max"),
                                          _torch_pool(x, "max", size, strides, padding).astype(F32))
            sums, cnt = _torch_pool(x, "avg", size, strides, padding)
            # the values are multiples of 2^-10 (or grid codes): the float64 sums are exact and fit float32
            assert np.array_equal(sums.astype(F32).astype(np.float64), sums)
            got = P.expected(gi, kind, C, bits, vset, "avg")
            np.testing.assert_array_equal(got, sums.astype(F32) / cnt.astype(F32))
            if vset == "const":                      # padding is not counted: a constant image stays the constant
                assert np.all(got == x.flat[0])
            if vset == "min":                        # ... and takes no part in a maximum
                assert np.all(P.expected(gi, kind, C, bits, vset, "max") == x.flat[0])


def test_the_case_list_holds_the_paddings_the_issue_names():
    pads = {}
    for g in P.GEOMS:
        N, H, W, size, strides, padding = P.geom(g)
        if padding == "same":
            s = size if strides is None else strides
            out, before = P.axis(H, size[0], s[0], True)
            total = max((out - 1) * s[0] + size[0] - H, 0)
            pads[(H, size[0], s[0])] = (before, total - before)
    assert pads[(8, 3, 2)] == (0, 1) and pads[(7, 3, 2)] == (1, 1) and pads[(8, 2, 2)] == (0, 0)


def test_output_sizes_are_the_convolutions_rule():
    for h in range(1, 12):
        for k in range(1, 5):
            for s in range(1, 5):
                assert P.axis(h, k, s, True)[0] == _abi.out_hw(h, k, s, True, 1)
                if k <= h:
                    assert P.axis(h, k, s, False)[0] == _abi.out_hw(h, k, s, False, 1)
    for gi, g in enumerate(P.GEOMS):
        N, H, W, size, strides, padding = P.geom(g)
        s = size if strides is None else strides
        same = padding == "same"
        want = (N, _abi.out_hw(H, size[0], s[0], same, 1), _abi.out_hw(W, size[1], s[1], same, 1), 5)
        assert P.expected(gi, "f32", 5, 0, "const", "max").shape == want


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_the_extension_header_and_the_exports():
    hdr = open(os.path.join(ROOT, "include", "qnn_abi_pool.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(qnn_[a-z0-9_]+)\s*\(", code))) == sorted(_abi.EXPORTS_POOL)
    assert sorted(_abi.EXPORTS_POOL) == ["qnn_pool2d_forward", "qnn_pool2d_out_hw"]
    assert re.search(r"#define QNN_POOL_MAX\s+0\b", hdr) and re.search(r"#define QNN_POOL_AVG\s+1\b", hdr)
    assert (_abi.POOL_MAX, _abi.POOL_AVG) == (0, 1)
    body = re.search(r"typedef struct qnn_pool2d \{([^{}]*)\} qnn_pool2d_t;", code).group(1)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.replace("int32_t", "").split(",")]
    assert fields == [n for n, _ in _abi.Pool2D._fields_] and ctypes.sizeof(_abi.Pool2D) == 24
    assert not set(_abi.EXPORTS_POOL) & set(_abi.EXPORTS + _abi.EXPORTS_QACT + _abi.EXPORTS_DILATION + _abi.EXPORTS_MAXACT)
    assert len(_abi.EXPORTS) == 29                   # qnn_abi.h's own list is what it was
    lib = ctypes.CDLL(_abi.lib_path())
    for n in _abi.EXPORTS_POOL:
        assert hasattr(lib, n), n
    assert _abi.load().qnn_version() == 4


def _desc(mode=0, size=(2, 2), strides=(2, 2), same=0):
    return _abi.Pool2D(mode, size[0], size[1], strides[0], strides[1], same)


def test_out_hw_entry():
    lib = _abi.load()
    ho, wo = ctypes.c_int(-7), ctypes.c_int(-7)
    for g in P.GEOMS:
        N, H, W, size, strides, padding = P.geom(g)
        d = _desc(0, size, size if strides is None else strides, int(padding == "same"))
        assert lib.qnn_pool2d_out_hw(H, W, ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) == 0
        s = size if strides is None else strides
        assert (ho.value, wo.value) == (P.axis(H, size[0], s[0], padding == "same")[0],
                                        P.axis(W, size[1], s[1], padding == "same")[0])
    bad = [(8, 8, None), (0, 8, _desc()), (8, -1, _desc()), (2, 8, _desc(size=(3, 3))), (8, 2, _desc(size=(3, 3))),
           (8, 8, _desc(strides=(0, 2))), (8, 8, _desc(strides=(2, 0))), (8, 8, _desc(size=(0, 2))), (8, 8, _desc(mode=2)),
           (8, 8, _desc(same=2)), (8, 8, _desc(size=(2, -3)))]
    for H, W, d in bad:
        rc = lib.qnn_pool2d_out_hw(H, W, ctypes.byref(d) if d is not None else None, ctypes.byref(ho), ctypes.byref(wo))
        assert rc == EINVAL, (H, W)
        assert _abi.load().qnn_last_error()
    assert lib.qnn_pool2d_out_hw(8, 8, ctypes.byref(_desc()), None, ctypes.byref(wo)) == EINVAL
    # 'same' takes a window larger than the image
    assert lib.qnn_pool2d_out_hw(2, 2, ctypes.byref(_desc(size=(3, 3), strides=(1, 1), same=1)), ctypes.byref(ho),
                                 ctypes.byref(wo)) == 0 and (ho.value, wo.value) == (2, 2)


def test_forward_refuses_bad_arguments_before_any_device_call():
    """No GPU here: every answer below is given before the first HIP call.  The pointers are never read."""
    lib = _abi.load()
    x, y = ctypes.c_void_p(1 << 40), ctypes.c_void_p(1 << 50)
    F, B, T2, I4, I8 = _abi.STORE_F32, _abi.STORE_BIN, _abi.STORE_T2, _abi.STORE_I4, _abi.STORE_I8

    def fwd(xs=I4, bits=4, N=1, H=8, W=8, C=8, d=None, ys=None, xp=x, yp=y, mode=0):
        d = _desc(mode=mode) if d is None else d
        ys = (xs if d.mode == 0 else F) if ys is None else ys
        return lib.qnn_pool2d_forward(xp, xs, bits, N, H, W, C, ctypes.byref(d), yp, ys, None)

    assert fwd(xp=None) == EINVAL and fwd(yp=None) == EINVAL                   # null pointers
    assert lib.qnn_pool2d_forward(x, I4, 4, 1, 8, 8, 8, None, y, I4, None) == EINVAL
    assert fwd(H=2, d=_desc(size=(3, 3))) == EINVAL                            # 'valid' window larger than the image
    assert fwd(d=_desc(strides=(0, 1))) == EINVAL and fwd(d=_desc(strides=(1, 0))) == EINVAL
    assert fwd(mode=1, ys=I4) == EINVAL and fwd(xs=B, bits=1, mode=1, ys=B) == EINVAL      # avg leaves the grid
    assert fwd(mode=0, ys=F) == EINVAL and fwd(xs=F, mode=0, ys=I4) == EINVAL   # max keeps the store
    assert fwd(xs=T2, bits=1) == EUNSUPPORTED and fwd(xs=T2, bits=1, mode=1) == EUNSUPPORTED
    assert b"QNN_STORE_T2" in lib.qnn_last_error()
    assert fwd(xs=I4, bits=5) == EINVAL and fwd(xs=I8, bits=9) == EINVAL and fwd(xs=I4, bits=0) == EINVAL
    assert fwd(xs=_abi.STORE_U8) == EINVAL and fwd(xs=3) == EINVAL
    assert fwd(C=0) == EINVAL and fwd(N=-1) == EINVAL and fwd(H=0) == EINVAL
    assert fwd(yp=x) == EINVAL and fwd(yp=ctypes.c_void_p((1 << 40) + 64)) == EINVAL       # x and y overlap
    assert b"overlap" in lib.qnn_last_error()
    assert fwd(xs=F, N=1 << 20, H=64, W=64, C=64, d=_desc(size=(1, 1), strides=(1, 1))) == EUNSUPPORTED    # 2^36 items
    # an empty batch is fine and launches nothing (the pointers may be null) -- but only with valid arguments
    assert fwd(N=0) == 0 and fwd(N=0, xp=None, yp=None) == 0 and fwd(N=0, xs=F, mode=1) == 0
    assert fwd(N=0, bits=7) == EINVAL and fwd(N=0, xs=T2) == EUNSUPPORTED


def test_the_binding_refuses_before_the_library():
    with pytest.raises(_abi.QnnError):
        _abi.pool2d(torch.zeros(1, 4, 4, 3), _abi.STORE_F32, 0, 1, 4, 4, 3, _abi.POOL_MAX, 2)         # a CPU tensor
    with pytest.raises(_abi.QnnError, match="larger than"):
        _abi.pool2d(torch.zeros(1, 2, 2, 3), _abi.STORE_F32, 0, 1, 2, 2, 3, _abi.POOL_MAX, 3)
    with pytest.raises(_abi.QnnUnsupported):
        _abi.pool2d(torch.zeros(4, 2, dtype=torch.int32), _abi.STORE_T2, 1, 1, 2, 2, 3, _abi.POOL_MAX, 2)


# ---- the layer classes ----------------------------------------------------------------------------------------------------
def test_layer_classes():
    for cls in (qnn_amd.MaxPooling2D, qnn_amd.AveragePooling2D):
        l = cls()
        assert (l.pool_size, l.strides, l.padding, l.data_format) == ((2, 2), (2, 2), "valid", "channels_last")
        assert l.compute_output_shape((None, 9, 6, 5)) == (None, 4, 3, 5)
        l = cls(3, strides=2, padding="same", name="p")
        assert (l.pool_size, l.strides, l.padding) == ((3, 3), (2, 2), "same")
        assert l.compute_output_shape((4, 8, 7, 16)) == (4, 4, 4, 16)
        assert cls((3, 2)).compute_output_shape((1, 9, 6, 2)) == (1, 3, 3, 2)
        assert cls((3, 2), strides=(1, 1)).compute_output_shape((1, None, 6, 2)) == (1, None, 5, 2)
        cfg = l.get_config()
        assert set(cfg) == {"name", "trainable", "pool_size", "padding", "strides", "data_format"}
        assert cls.from_config(cfg).get_config() == cfg and cfg["name"] == "p"
        with pytest.raises(ValueError, match=r'The `padding` argument must be one of "valid", "same"\. Received: full'):
            cls(padding="full")
        with pytest.raises(ValueError, match="`pool_size` argument must be a tuple of 2 integers"):
            cls(pool_size=(2, 2, 2))
        with pytest.raises(_abi.QnnError, match="channels_last"):
            cls(data_format="channels_first")
        with pytest.raises(_abi.QnnError):
            cls()(torch.zeros(1, 4, 4, 3))                    # a CPU tensor: no CPU path
    for cls in (qnn_amd.GlobalAveragePooling2D, qnn_amd.GlobalMaxPooling2D):
        l = cls(name="g")
        assert l.compute_output_shape((None, 7, 7, 64)) == (None, 64)
        cfg = l.get_config()
        assert set(cfg) == {"name", "trainable", "data_format"} and cls.from_config(cfg).get_config() == cfg
        with pytest.raises(_abi.QnnError, match="channels_last"):
            cls(data_format="channels_first")
        with pytest.raises(_abi.QnnError):
            cls()(torch.zeros(1, 4, 4, 3))
    for n in ("MaxPooling2D", "AveragePooling2D", "GlobalAveragePooling2D", "GlobalMaxPooling2D"):
        assert n in qnn_amd.__all__


# ---- the importer ---------------------------------------------------------------------------------------------------------
def _npz(tmp_path, layers):
    cfg = {"class_name": "Model", "config": {"layers": [
        {"class_name": "InputLayer", "name": "in", "config": {}, "inbound_nodes": []}]}}
    prev = "in"
    for i, (cls, c) in enumerate(layers):
        name = "l%d" % i
        cfg["config"]["layers"].append({"class_name": cls, "name": name, "config": dict(c, name=name),
                                        "inbound_nodes": [[[prev, 0, 0, {}]]]})
        prev = name
    path = tmp_path / "m.npz"
    np.savez(path, model_config_json=np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8))
    return str(path)


def _pool_cfg(size, strides=None, padding="valid", data_format="channels_last"):
    return {"pool_size": list(size), "strides": None if strides is None else list(strides), "padding": padding,
            "data_format": data_format, "trainable": True}


def test_importer_reads_the_whole_pooling_config(tmp_path):
    spec = nets.spec_from_keras_npz(_npz(tmp_path, [
        ("MaxPooling2D", _pool_cfg((2, 2), (2, 2))),                     # what MaxPooling2D() serialises
        ("MaxPooling2D", _pool_cfg((3, 3), (2, 2), "same")),
        ("AveragePooling2D", _pool_cfg((3, 2), (3, 2))),
        ("AveragePooling2D", _pool_cfg((8, 8), None)),
        ("MaxPooling2D", _pool_cfg((2, 2), (1, 1))),
        ("GlobalAveragePooling2D", {"data_format": "channels_last"}),
    ]))
    assert spec[0] == {"op": "maxpool", "size": 2, "src": "input", "dst": "l0"}      # element for element what it was
    assert type(spec[0]["size"]) is int and not engine._new_pool(spec[0])
    assert spec[1] == {"op": "maxpool", "size": (3, 3), "strides": (2, 2), "padding": "same", "src": "l0", "dst": "l1"}
    assert spec[2] == {"op": "avgpool", "size": (3, 2), "strides": (3, 2), "padding": "valid", "src": "l1", "dst": "l2"}
    assert spec[3] == {"op": "avgpool", "size": 8, "src": "l2", "dst": "l3"}
    assert spec[4] == {"op": "maxpool", "size": (2, 2), "strides": (1, 1), "padding": "valid", "src": "l3", "dst": "l4"}
    assert spec[5] == {"op": "globalavgpool", "src": "l4", "dst": "l5"}
    assert [engine._new_pool(op) for op in spec] == [False, True, True, False, True, True]
    spec = nets.spec_from_keras_npz(_npz(tmp_path, [("GlobalMaxPooling2D", {})]))
    assert spec == [{"op": "globalmaxpool", "src": "input", "dst": "l0"}]
    for cls, c in (("MaxPooling2D", _pool_cfg((2, 2), data_format="channels_first")),
                   ("AveragePooling2D", _pool_cfg((2, 2), data_format="channels_first")),
                   ("GlobalAveragePooling2D", {"data_format": "channels_first"}),
                   ("GlobalMaxPooling2D", {"data_format": "channels_first"})):
        with pytest.raises(ValueError, match="channels_first"):
            nets.spec_from_keras_npz(_npz(tmp_path, [(cls, c)]))


# ---- the engines' reading of the ops --------------------------------------------------------------------------------------
def _chain(pool):
    rng = np.random.default_rng(3)
    conv = {"op": "conv", "kind": "quantized", "nb": 4, "kernel": rng.uniform(-1, 1, (3, 3, 3, 8)).astype(F32), "bias": None,
            "strides": (1, 1), "padding": "same"}
    dense = {"op": "dense", "kind": "quantized", "nb": 4, "kernel": rng.uniform(-1, 1, (8 * 16, 10)).astype(F32), "bias": None}
    return [conv, {"op": "act", "fn": "quantized_tanh", "nb": 4}, pool, {"op": "flatten"}, dense]


def test_old_and_new_forms():
    assert not engine._new_pool({"op": "maxpool", "size": 2}) and not engine._new_pool({"op": "avgpool", "size": 8})
    assert not engine._new_pool({"op": "maxpool"}) and not engine._new_pool({"op": "avgpool", "size": np.int64(4)})
    for op in ({"op": "maxpool", "size": 2, "strides": (1, 1)}, {"op": "maxpool", "size": 2, "padding": "valid"},
               {"op": "maxpool", "size": (2, 2)}, {"op": "avgpool", "size": 8, "padding": "same"},
               {"op": "globalavgpool"}, {"op": "globalmaxpool"}):
        assert engine._new_pool(op), op
    assert not engine._new_pool({"op": "conv", "strides": (1, 1), "padding": "same"})
    assert set(engine._POOLS) <= set(engine._GLUE)


@pytest.mark.parametrize("pool", [{"op": "maxpool", "size": 2, "strides": (1, 1)}, {"op": "maxpool", "size": 2, "padding": "same"},
                                  {"op": "maxpool", "size": (2, 2)}, {"op": "maxpool", "size": 3, "strides": (2, 2), "padding": "same"}])
def test_the_chain_engine_refuses_a_new_form_pool(pool):
    """Fusing it as the 2x2 / 2 epilogue pool would be a wrong answer; the refusal comes before any weights are packed."""
    assert engine.FusedModel._group(_chain({"op": "maxpool", "size": 2})) is not None
    assert engine.FusedModel._group(_chain(pool)) is None
    with pytest.raises(_abi.NotFusable):
        engine.FusedModel(_chain(pool))


def test_the_fused_classifier_tail_takes_the_old_form_only():
    rng = np.random.default_rng(4)
    dense = {"op": "dense", "kind": "float", "kernel": rng.uniform(-1, 1, (8, 10)).astype(F32), "bias": None}
    for pool, fused in (({"op": "avgpool", "size": 8}, True), ({"op": "avgpool", "size": 8, "padding": "valid"}, False),
                        ({"op": "avgpool", "size": (8, 8)}, False), ({"op": "globalavgpool"}, False)):
        spec = [{"op": "act", "fn": "quantized_tanh", "nb": 4}, pool, {"op": "flatten"}, dense, {"op": "softmax"}]
        g = engine._SpecGraph.__new__(engine._SpecGraph)
        g.spec, g.names = spec, ["t%d" % i for i in range(len(spec))]
        g.prod = {n: i for i, n in enumerate(g.names)}
        g.srcs = [["input"]] + [[g.names[i - 1]] for i in range(1, len(spec))]
        g.cons = {s[0]: [i] for i, s in enumerate(g.srcs)}
        g.tails = {}
        assert (g.tail(4) is not None) == fused, pool
        assert (g.tail_from(1) is not None) == fused, pool


def test_the_residual_engine_looks_through_a_new_form_max_pool():
    """The activation in front of a new-form max-pool is stored packed for the contraction behind the pool; in front of
    an old-form one it is float32, as before."""
    def spec(pool):
        rng = np.random.default_rng(5)
        k = lambda ci, co: rng.uniform(-1, 1, (3, 3, ci, co)).astype(F32)
        q = {"op": "act", "fn": "quantized_tanh", "nb": 4}
        return [{"op": "conv", "kind": "quantized", "nb": 4, "kernel": k(8, 8), "bias": None}, dict(q), pool,
                {"op": "conv", "kind": "quantized", "nb": 4, "kernel": k(8, 8), "bias": None}, dict(q), {"op": "globalavgpool"}]

    def model(s):
        m = engine.ResidualFusedModel.__new__(engine.ResidualFusedModel)
        m.spec = s
        m.names = ["t%d" % i for i in range(len(s))]
        m.prod = {n: i for i, n in enumerate(m.names)}
        m.srcs = [["input"]] + [[m.names[i - 1]] for i in range(1, len(s))]
        m.cons = {}
        for i, ss in enumerate(m.srcs):
            m.cons.setdefault(ss[0], []).append(i)
        return m
    m = model(spec({"op": "maxpool", "size": 3, "strides": (2, 2), "padding": "same"}))
    assert m._act_out_store("t1", 4) == _abi.STORE_I4 and m._act_out_store("t4", 4) == _abi.STORE_I4
    m = model(spec({"op": "globalmaxpool"}))
    assert m._act_out_store("t1", 4) == _abi.STORE_I4
    m = model(spec({"op": "maxpool", "size": 2}))
    assert m._act_out_store("t1", 4) is None
    s = spec({"op": "maxpool", "size": (2, 2)})
    s[3] = {"op": "bn"}                                   # a float32 consumer behind the pool: float32 in front of it
    assert model(s)._act_out_store("t1", 4) is None
    assert [u["op"] for u in model(spec({"op": "globalmaxpool"}))._users_through_pools("t1")] == ["conv"]
