"""ZeroPadding2D, Cropping2D and UpSampling2D without a GPU: the extension header and its argument checks (no device is
touched before them), the numpy reference of spatial_cases.py against torch on CPU float32, the output-size entry on every
case, the layer classes' argument forms, the checkpoint importer and the refusal of the fused engines."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi, engine, nets

import spatial_cases as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
EINVAL, EUNSUPPORTED = -1, -2
ENTRIES = _abi.EXPORTS_SPATIAL           # read at import: without the entries, the ops and the classes nothing below means anything
LAYERS = (qnn_amd.ZeroPadding2D, qnn_amd.Cropping2D, qnn_amd.UpSampling2D)


def cdesc(d):
    return _abi.spatial_desc(d["crop"], d["up"], d["pad"])


ALL_DESCS = [(hw, d) for _, hw, d in Z.DESCS] + [(Z.RAGGED_IMAGE, d) for _, _, d in Z.DESCS] + [((3, 5), Z.IDENTITY)]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_the_extension_header_and_the_exports():
    hdr = open(os.path.join(ROOT, "include", "qnn_abi_spatial.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(qnn_[a-z0-9_]+)\s*\(", code))) == sorted(_abi.EXPORTS_SPATIAL)
    assert _abi.EXPORTS_SPATIAL == ["qnn_spatial2d_out_hw", "qnn_spatial2d_forward"]
    body = re.search(r"typedef struct qnn_spatial2d \{([^{}]*)\} qnn_spatial2d_t;", code).group(1)
    fields = [re.sub(r"\[.*\]", "", d.split()[-1]) for d in body.split(";") if d.strip()]
    assert fields == [n for n, _ in _abi.Spatial2D._fields_] == ["crop", "up", "pad"]
    assert ctypes.sizeof(_abi.Spatial2D) == 4 * 10
    others = _abi.EXPORTS + _abi.EXPORTS_QACT + _abi.EXPORTS_DILATION + _abi.EXPORTS_MAXACT + _abi.EXPORTS_POOL + \
        _abi.EXPORTS_SCALED + _abi.EXPORTS_CONCAT
    assert not set(_abi.EXPORTS_SPATIAL) & set(others)
    assert len(_abi.EXPORTS) == 29                   # qnn_abi.h's own list is what it was
    lib = ctypes.CDLL(_abi.lib_path())
    assert all(hasattr(lib, n) for n in _abi.EXPORTS_SPATIAL)
    assert _abi.load().qnn_version() == 4


def test_out_hw_on_every_case():
    for (H, W), d in ALL_DESCS:
        assert _abi.spatial2d_out_hw(H, W, d["crop"], d["up"], d["pad"]) == Z.out_hw(H, W, d), (H, W, d)
    assert Z.out_hw(3, 5, Z.DESCS[0][2]) == (6, 8) and Z.out_hw(4, 6, Z.DESCS[1][2]) == (3, 3)
    assert Z.out_hw(3, 5, Z.DESCS[2][2]) == (6, 15) and Z.out_hw(4, 6, Z.DESCS[4][2]) == (9, 12)
    lib = _abi.load()
    ho, wo = ctypes.c_int(0), ctypes.c_int(0)

    def hw(H=4, W=6, d=Z.IDENTITY, desc="make", out=(ho, wo)):
        desc = cdesc(d) if desc == "make" else desc
        rc = lib.qnn_spatial2d_out_hw(H, W, ctypes.byref(desc) if desc is not None else None,
                                      ctypes.byref(out[0]) if out[0] is not None else None,
                                      ctypes.byref(out[1]) if out[1] is not None else None)
        if rc != 0:
            assert b"qnn_spatial2d_out_hw" in lib.qnn_last_error()
        return rc

    assert hw() == 0 and (ho.value, wo.value) == (4, 6)
    assert hw(desc=None) == EINVAL and hw(out=(None, wo)) == EINVAL and hw(out=(ho, None)) == EINVAL
    assert hw(H=0) == EINVAL and hw(W=0) == EINVAL and hw(H=-1) == EINVAL
    assert hw(d=Z.desc(crop=((-1, 0), (0, 0)))) == EINVAL and hw(d=Z.desc(pad=((0, 0), (0, -1)))) == EINVAL
    assert hw(d=Z.desc(up=(0, 1))) == EINVAL and hw(d=Z.desc(up=(1, 0))) == EINVAL
    assert hw(d=Z.desc(crop=((2, 2), (0, 0)))) == EINVAL and b"no row" in lib.qnn_last_error()
    assert hw(d=Z.desc(crop=((0, 0), (3, 3)))) == EINVAL and b"no column" in lib.qnn_last_error()
    assert hw(d=Z.desc(crop=((2, 1), (3, 2)))) == 0 and (ho.value, wo.value) == (1, 1)
    assert hw(H=1 << 30, d=Z.desc(up=(4, 1))) == EUNSUPPORTED


def test_forward_refuses_bad_arguments_before_any_device_call():
    """No GPU here: every answer below is given before the first HIP call.  The pointers are never read."""
    lib = _abi.load()
    X, Y = ctypes.c_void_p(1 << 40), ctypes.c_void_p(1 << 50)
    F, B, T2, I4, I8 = _abi.STORE_F32, _abi.STORE_BIN, _abi.STORE_T2, _abi.STORE_I4, _abi.STORE_I8

    def fwd(store=I4, bits=4, N=2, H=4, W=6, C=9, d=Z.IDENTITY, x=X, y=Y, desc="make"):
        desc = cdesc(d) if desc == "make" else desc
        rc = lib.qnn_spatial2d_forward(x, store, bits, N, H, W, C, ctypes.byref(desc) if desc is not None else None, y, None)
        if rc != 0:
            assert b"qnn_spatial2d_forward" in lib.qnn_last_error(), lib.qnn_last_error()    # every message names the entry
        return rc

    assert fwd(desc=None) == EINVAL                                                   # null descriptor
    assert fwd(x=None) == EINVAL and fwd(y=None) == EINVAL and b"null" in lib.qnn_last_error()
    assert fwd(H=0) == EINVAL and fwd(W=0) == EINVAL and fwd(C=0) == EINVAL and fwd(C=-3) == EINVAL and fwd(N=-1) == EINVAL
    assert fwd(d=Z.desc(crop=((0, -1), (0, 0)))) == EINVAL and fwd(d=Z.desc(pad=((-2, 0), (0, 0)))) == EINVAL
    assert fwd(d=Z.desc(up=(0, 2))) == EINVAL and fwd(d=Z.desc(up=(2, -1))) == EINVAL
    assert fwd(d=Z.desc(crop=((1, 3), (0, 0)))) == EINVAL and fwd(d=Z.desc(crop=((0, 0), (6, 0)))) == EINVAL
    for store in (3, 5, _abi.STORE_U8, _abi.STORE_F32_IMAGE, _abi.STORE_F32_UNIT, -1):
        assert fwd(store=store) == EINVAL, store
    assert fwd(store=I4, bits=5) == EINVAL and fwd(store=I4, bits=0) == EINVAL and fwd(store=I8, bits=9) == EINVAL
    # y overlapping x: the same address, inside it, x beginning inside y; side by side is fine up to the pointers
    nbytes = 2 * 4 * 6 * 2 * 4                                                        # I4, 9 channels: two words a pixel
    assert fwd(y=X) == EINVAL and b"overlap" in lib.qnn_last_error()
    assert fwd(y=ctypes.c_void_p((1 << 40) + nbytes - 4)) == EINVAL
    assert fwd(y=ctypes.c_void_p((1 << 40) - nbytes + 4)) == EINVAL
    # a +-1 code has no zero
    for pad in (((1, 0), (0, 0)), ((0, 1), (0, 0)), ((0, 0), (1, 0)), ((0, 0), (0, 1))):
        assert fwd(store=B, bits=1, d=Z.desc(pad=pad)) == EUNSUPPORTED
        msg = lib.qnn_last_error().decode()
        assert "no zero" in msg and "unpack, pad in float32" in msg
    # 2^31 words or more
    assert fwd(store=F, bits=0, N=1 << 15, H=1 << 8, W=1 << 8, C=1) == EUNSUPPORTED
    assert fwd(store=I4, N=1 << 10, H=1 << 10, W=1 << 9, C=9, d=Z.desc(up=(1, 2))) == EUNSUPPORTED
    assert fwd(store=B, bits=1, N=1, H=1 << 15, W=1 << 15, C=33, d=Z.desc(up=(1, 1))) == EUNSUPPORTED
    # N == 0: QNN_OK without a launch, the pointers may be null
    assert fwd(N=0, x=None, y=None) == 0 and fwd(N=0, store=T2, bits=1, d=Z.DESCS[4][2]) == 0
    # the binding
    with pytest.raises(_abi.QnnError, match="no CPU path"):
        _abi.spatial2d(torch.zeros(1, 3, 5, 2), F, 0, 1, 3, 5, 2, pad=1)
    with pytest.raises(_abi.QnnError, match="contiguous int32 CUDA"):
        _abi.spatial2d(torch.zeros(15, 1, dtype=torch.int32), I4, 4, 1, 3, 5, 2, pad=1)
    with pytest.raises(_abi.QnnError, match="no row"):
        _abi.spatial2d(torch.zeros(1, 3, 5, 2), F, 0, 1, 3, 5, 2, crop=((2, 1), (0, 0)))


# ---- the reference --------------------------------------------------------------------------------------------------------
def test_the_reference_is_torch_pad_slice_and_repeat_interleave():
    for (H, W), d in ALL_DESCS:
        x = Z.f32_values(2 * H * W, 3, 5).reshape(2, H, W, 3)
        t = torch.from_numpy(np.array(x))
        (ct, cb), (cl, cr) = d["crop"]
        (pt, pb), (pl, pr) = d["pad"]
        t = t[:, ct:H - cb, cl:W - cr]
        t = t.repeat_interleave(d["up"][0], dim=1).repeat_interleave(d["up"][1], dim=2)
        t = torch.nn.functional.pad(t, (0, 0, pl, pr, pt, pb))
        got = Z.spatial_ref(x.reshape(-1, 3), "f32", (2, H, W, 3), d)
        assert got.shape == (2,) + Z.out_hw(H, W, d) + (3,)
        np.testing.assert_array_equal(got.view(np.uint32), t.numpy().view(np.uint32))


def test_the_packed_reference_moves_codes_and_clears_the_spare_bits():
    for kind in ("bin", "t2", "i4", "i8"):
        for Cn in [c for c in Z.CHANNELS[kind] if c]:
            for _, (H, W), d in Z.DESCS:
                if kind == "bin" and Z.padded(d):
                    continue
                bits = Z.BITS[kind][-1]
                k = Z.codes(kind, bits, 2 * H * W, Cn, 3)
                w = Z.encode(k, kind)
                got = Z.spatial_ref(w | Z.spare(kind, Cn), kind, (2, H, W, Cn), d)
                np.testing.assert_array_equal(got, Z.spatial_ref(w, kind, (2, H, W, Cn), d))
                assert not np.any(got & Z.spare(kind, Cn))
                want = Z.spatial_array(k.reshape(2, H, W, Cn), d)
                np.testing.assert_array_equal(Z.decode(got, kind, Cn).reshape(want.shape), want)
    assert Z.form("i4", 32) == "v4" and Z.form("i4", 32, aligned16=False) == "v1" and Z.form("i4", 8) == "v1"
    assert Z.form("t2", 64) == "v4" and Z.form("t2", 33) == "v4" and Z.form("t2", 32) == "v1" and Z.form("f32", 4) == "v4" and Z.form("bin", 128) == "v4"


# ---- the layer classes ------------------------------------------------------------------------------------------------------
def test_the_layers_take_keras_argument_forms():
    assert qnn_amd.ZeroPadding2D().padding == ((1, 1), (1, 1))
    assert qnn_amd.ZeroPadding2D(2).padding == ((2, 2), (2, 2))
    assert qnn_amd.ZeroPadding2D((1, 3)).padding == ((1, 1), (3, 3))
    assert qnn_amd.ZeroPadding2D(((1, 2), (0, 3))).padding == ((1, 2), (0, 3))
    assert qnn_amd.Cropping2D().cropping == ((0, 0), (0, 0))
    assert qnn_amd.Cropping2D(1).cropping == ((1, 1), (1, 1))
    assert qnn_amd.Cropping2D((1, 2)).cropping == ((1, 1), (2, 2))
    assert qnn_amd.Cropping2D(((1, 0), (2, 1))).cropping == ((1, 0), (2, 1))
    assert qnn_amd.UpSampling2D().size == (2, 2) and qnn_amd.UpSampling2D(3).size == (3, 3)
    assert qnn_amd.UpSampling2D((2, 3)).size == (2, 3)
    assert qnn_amd.ZeroPadding2D(((1, 2), (0, 3))).compute_output_shape((None, 3, 5, 7)) == (None, 6, 8, 7)
    assert qnn_amd.Cropping2D(((1, 0), (2, 1))).compute_output_shape((None, 4, 6, 7)) == (None, 3, 3, 7)
    assert qnn_amd.UpSampling2D((2, 3)).compute_output_shape((4, 3, 5, 7)) == (4, 6, 15, 7)
    for cls, bad in ((qnn_amd.ZeroPadding2D, (1, 2, 3)), (qnn_amd.ZeroPadding2D, "same"), (qnn_amd.ZeroPadding2D, ((1, 2, 3), (0, 0))),
                     (qnn_amd.ZeroPadding2D, -1), (qnn_amd.Cropping2D, (1,)), (qnn_amd.Cropping2D, ((0, -1), (0, 0))),
                     (qnn_amd.UpSampling2D, (1, 2, 3)), (qnn_amd.UpSampling2D, 0)):
        with pytest.raises(ValueError):
            cls(bad)
    for cls in LAYERS:
        assert cls(data_format="channels_last").data_format == "channels_last"
        with pytest.raises(ValueError, match="channels_last"):
            cls(data_format="channels_first")
        with pytest.raises(ValueError):
            cls(data_format="nchw")
        with pytest.raises(_abi.QnnError, match="no CPU path"):
            cls()(torch.zeros(1, 4, 4, 2))
        layer = cls.from_config(cls().get_config())
        assert layer.get_config() == cls().get_config()
    assert qnn_amd.UpSampling2D(interpolation="nearest").size == (2, 2)
    with pytest.raises(ValueError, match="nearest"):
        qnn_amd.UpSampling2D(interpolation="bilinear")
    with pytest.raises(_abi.QnnError, match="no row"):
        qnn_amd.Cropping2D(2).compute_output_shape((None, 4, 6, 1))


# ---- the importer ------------------------------------------------------------------------------------------------------
def _npz(tmp_path, layers):
    """A hand-written Keras 2.1.3 functional model_config around `layers` = [(class, config)], chained."""
    ls, prev = [{"class_name": "InputLayer", "name": "in", "config": {"name": "in", "batch_input_shape": [None, 8, 8, 3]},
                 "inbound_nodes": []}], "in"
    for i, (cls, cfg) in enumerate(layers):
        name = "l%d" % i
        ls.append({"class_name": cls, "name": name, "config": dict(cfg, name=name), "inbound_nodes": [[[prev, 0, 0, {}]]]})
        prev = name
    cfg = {"class_name": "Model", "config": {"name": "m", "layers": ls, "input_layers": [["in", 0, 0]],
                                             "output_layers": [[prev, 0, 0]]}}
    path = os.path.join(str(tmp_path), "m.npz")
    np.savez(path, model_config_json=np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8))
    return path


def test_the_importer_reads_all_four_numbers(tmp_path):
    spec = nets.spec_from_keras_npz(_npz(tmp_path, [
        ("ZeroPadding2D", {"padding": [[1, 2], [0, 3]], "data_format": "channels_last"}),
        ("ZeroPadding2D", {"padding": [[2, 2], [2, 2]]}),
        ("ZeroPadding2D", {"padding": [[1, 1], [2, 2]]}),
        ("Cropping2D", {"cropping": [[1, 0], [2, 1]]}),
        ("UpSampling2D", {"size": [2, 3]}),
    ]))
    ops = [{k: v for k, v in op.items() if k not in ("src", "dst")} for op in spec]
    assert ops == [{"op": "zeropad", "pad": ((1, 2), (0, 3))}, {"op": "zeropad", "pad": 2},
                   {"op": "zeropad", "pad": ((1, 1), (2, 2))}, {"op": "crop", "crop": ((1, 0), (2, 1))},
                   {"op": "upsample", "size": (2, 3)}]
    assert isinstance(ops[1]["pad"], int)                # the integer form the shipped checkpoints' specs carry
    assert [engine._new_spatial(op) for op in spec] == [True, False, True, True, True]
    for cls, cfg in (("ZeroPadding2D", {"padding": [[1, 1], [1, 1]]}), ("Cropping2D", {"cropping": [[1, 1], [1, 1]]}),
                     ("UpSampling2D", {"size": [2, 2]})):
        with pytest.raises(ValueError, match="channels_first"):
            nets.spec_from_keras_npz(_npz(tmp_path, [(cls, dict(cfg, data_format="channels_first"))]))
    with pytest.raises(ValueError, match="nearest"):
        nets.spec_from_keras_npz(_npz(tmp_path, [("UpSampling2D", {"size": [2, 2], "interpolation": "bilinear"})]))


# ---- the engines ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Z.SPECS) + ["chain_" + n for n in Z.CHAINS])
def test_the_fused_engines_refuse_by_name(name):
    spec = (Z.CHAINS[name[6:]] if name.startswith("chain_") else Z.SPECS[name])[0].spec
    new = [op["op"] for op in spec if op["op"] in engine._SPATIAL and engine._new_spatial(op)]
    assert new
    if not any(op["op"] == "concat" for op in spec):
        for cls in (engine.FusedModel, engine.ResidualFusedModel):
            with pytest.raises(_abi.NotFusable, match="%s.*GraphModel" % new[0]):
                cls(spec)
    else:
        for cls in (engine.FusedModel, engine.ResidualFusedModel):
            with pytest.raises(_abi.NotFusable, match="GraphModel"):
                cls(spec)


def test_the_integer_zeropad_is_the_old_form():
    assert not engine._new_spatial({"op": "zeropad", "pad": 2}) and not engine._new_spatial({"op": "zeropad", "pad": np.int64(1)})
    assert engine._new_spatial({"op": "zeropad", "pad": ((2, 2), (2, 2))})
    t = torch.arange(2 * 3 * 5 * 2, dtype=torch.float32).reshape(2, 3, 5, 2)
    y = engine._GLUE["zeropad"](t, {"op": "zeropad", "pad": 2})          # torch on whatever device the tensor is on, as before
    assert y.shape == (2, 7, 9, 2) and torch.equal(y[:, 2:5, 2:7], t) and float(y.sum()) == float(t.sum())
    with pytest.raises(ValueError, match="top, bottom"):
        engine._spatial_steps({"op": "zeropad", "pad": (1, 2)})
    assert engine._spatial_steps({"op": "crop", "crop": ((1, 0), (2, 1))}) == {"crop": ((1, 0), (2, 1))}
    assert engine._spatial_steps({"op": "upsample", "size": (2, 3)}) == {"up": (2, 3)}
