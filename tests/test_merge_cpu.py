"""The merge layers without a GPU: the reference of merge_cases.py (the code rules against decode -> float32 chain ->
encode, the float32-out forms against exact integer arithmetic, the avg cases that tell a division from a multiplication
by the reciprocal), the extension header, its ctypes mirror and the argument checks (no device is touched before them),
the six layer classes, the checkpoint importer, the spec graph's reading of the op and the refusal of the fused engines."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi, engine, nets

import concat_cases as C
import merge_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
EINVAL, EUNSUPPORTED = -1, -2
ENTRIES = _abi.EXPORTS_MERGE             # read at import: without the entries, the op and the classes nothing below means anything
LAYERS = {"add": qnn_amd.Add, "sub": qnn_amd.Subtract, "mul": qnn_amd.Multiply, "avg": qnn_amd.Average,
          "max": qnn_amd.Maximum, "min": qnn_amd.Minimum}


@pytest.fixture(scope="module", autouse=True)
def _drop_the_case_tables():
    """The cached codes and operands are shared by the tests of this file and freed behind the last one."""
    yield
    M.codes.cache_clear()
    M.f32_inputs.cache_clear()


# ---- the reference ------------------------------------------------------------------------------------------------------
def test_the_case_tables_are_the_issues():
    assert M.CHANNELS == {"bin": (3, 32, 33, 128), "i4": (5, 8, 12, 64), "i8": (3, 4, 6, 16), "t2": (3, 32, 33),
                          "f32": (1, 3, 4, 7)}
    assert M.PIXELS == (1, 5, 64, 257, 2051) and M.NS == (2, 3, 8) and M.AVG_NS == (3, 5, 6, 7)
    assert M.BITS["i4"] == (2, 3, 4) and M.BITS["i8"] == (5, 8)
    assert M.OP_CODE == _abi.MERGE_OPS and M.MAX_INPUTS == _abi.MERGE_MAX
    assert sorted(M.PACKED_OUT) == sorted([("max", k) for k in ("bin", "i4", "i8", "t2")] + [("min", k) for k in ("bin", "i4", "i8", "t2")]
                                          + [("mul", "bin"), ("mul", "t2")])
    assert sorted(M.F32_OUT) == sorted([(op, k) for op in ("add", "sub", "avg") for k in ("bin", "i4", "i8", "t2")]
                                       + [("mul", "i4"), ("mul", "i8")])
    for kind, chans in M.CHANNELS.items():
        if kind != "f32":                # each store has a ragged last word and a full one
            assert any(M.spare(kind, c).any() for c in chans) and any(not M.spare(kind, c).any() for c in chans), kind
    for kind in ("i4", "i8"):            # both extreme codes in every tensor
        for bits in M.BITS[kind]:
            for seed in range(8):
                k = M.codes(kind, bits, 1, M.CHANNELS[kind][0], seed)
                assert k.min() == -(1 << (bits - 1)) and k.max() == (1 << (bits - 1)) - 1


def test_both_kernel_forms_are_reached_by_every_family():
    """The case table reaches the 16-byte and the 4-byte form of every kernel family with aligned pointers already (the GPU
    file moves the pointers as well, which is always the 4-byte form)."""
    for op, kind in M.PACKED_OUT + M.F32_OUT + [(op, "f32") for op in M.OPS]:
        seen = {M.form(op, kind, c, p) for c in M.CHANNELS[kind] for p in M.PIXELS}
        assert seen == {4, 16}, (op, kind, seen)
        assert all(M.form(op, kind, c, p, aligned16=False) == 4 for c in M.CHANNELS[kind] for p in M.PIXELS)
    assert M.form("max", "bin", 128, 2051) == 16 and M.form("max", "bin", 32, 2051) == 4 and M.form("max", "bin", 32, 64) == 16
    assert M.form("max", "bin", 33, 64) == 4 and M.form("max", "t2", 32, 5) == 4 and M.form("max", "t2", 32, 64) == 16
    assert M.form("add", "i4", 12, 5) == 16 and M.form("add", "i4", 5, 64) == 4 and M.form("add", "f32", 3, 64) == 16
    assert M.form("add", "f32", 3, 5) == 4 and M.form("add", "f32", 4, 2051) == 16


@pytest.mark.parametrize("kind", ["bin", "t2", "i4", "i8"])
def test_the_layout_is_concat_cases(kind):
    for c in M.CHANNELS[kind]:
        for bits in M.BITS[kind]:
            k = M.codes(kind, bits, 5, c, 1)
            w = M.encode(k, kind)
            assert w.shape == (5, M.words(kind, c)) == (5, C.words(kind, c))
            np.testing.assert_array_equal(w, C.encode(k, kind))
            np.testing.assert_array_equal(M.decode(w, kind, c), k)
            np.testing.assert_array_equal(M.decode(w | M.spare(kind, c), kind, c), k)        # the spare bits are not read
            np.testing.assert_array_equal(M.spare(kind, c), C.spare(kind, c))
            np.testing.assert_array_equal(M.to_codes(M.values(k, kind, bits), kind, bits), k)


@pytest.mark.parametrize("op,kind", M.PACKED_OUT)
def test_the_code_rules_are_decode_chain_encode(op, kind):
    """ref_codes equals decode -> ref_f32 -> encode: the packed-out forms need no arithmetic on values."""
    for c in M.CHANNELS[kind]:
        for bits in M.BITS[kind]:
            for n in M.ns_of(op):
                ks = [M.codes(kind, bits, 5, c, i) for i in range(n)]
                got = M.ref_codes(op, kind, bits, ks)
                chain = M.ref_f32(op, [M.values(M.decode(M.encode(k, kind), kind, c), kind, bits) for k in ks])
                np.testing.assert_array_equal(M.encode(got, kind), M.encode(M.to_codes(chain, kind, bits), kind))
                assert not np.any(M.encode(got, kind) & M.spare(kind, c))
    if kind == "t2" and op == "mul":     # the sign plane holds "is +1": the product's sign bit is the XNOR of the signs
        a, b = np.array([[1, 1, -1, -1, 0, 1]]), np.array([[1, -1, 1, -1, 1, 0]])
        np.testing.assert_array_equal(M.ref_codes("mul", "t2", 1, [a, b]), [[1, -1, -1, 1, 0, 0]])
        wa, wb, wy = (M.encode(k, "t2")[0] for k in (a, b, a * b))
        assert wy[0] == wa[0] & wb[0] and wy[1] == ~(wa[1] ^ wb[1]) & wy[0]


@pytest.mark.parametrize("op,kind", M.F32_OUT)
def test_the_float32_out_forms_are_exact_before_the_division(op, kind):
    """The decoded values are small dyadic numbers: the float32 chain on them equals the exact result in integers (for avg:
    the sum, before its one division), so decoding in registers is bit-identical to unpack -> the float32 form.  A product
    is held to this while its n * bits significant bits fit float32's 24; a longer one rounds, in both routes alike."""
    for c in M.CHANNELS[kind][:2]:
        for bits in M.BITS[kind]:
            for n in M.ns_of(op):
                ks = [M.codes(kind, bits, 64, c, i) for i in range(n)]
                xs = [M.values(k, kind, bits) for k in ks]
                unit = 1 if kind in ("bin", "t2") else 1 << (bits - 1)
                if op == "mul":
                    if n * bits > 24:
                        continue
                    exact, scale = np.multiply.reduce(ks), unit ** n
                else:
                    exact, scale = (ks[0] - ks[1] if op == "sub" else np.add.reduce(ks)), unit
                chain = M.ref_f32("add" if op == "avg" else op, xs).astype(np.float64) * scale
                assert all(int(a) == int(b) and float(a) == float(int(b)) for a, b in zip(chain.ravel(), exact.ravel()))
                if op == "avg":
                    want = (exact.astype(np.float64) / scale).astype(F32) / F32(n)
                    assert M.same_f32(M.ref_f32("avg", xs), want)


@pytest.mark.parametrize("n", M.AVG_NS)
def test_avg_cases_tell_a_division_from_a_reciprocal(n):
    for c in M.CHANNELS["f32"]:
        xs = M.f32_inputs("avg", n, 64, c)
        s = M.ref_f32("add", xs)
        div, mul = s / F32(n), s * (F32(1) / F32(n))
        assert div.dtype == mul.dtype == F32 and M.same_f32(M.ref_f32("avg", xs), div)
        assert np.any(div != mul), (n, c)


def test_float32_operands_and_the_special_pairs():
    for op in M.OPS:
        for n in M.ns_of(op):
            xs = M.f32_inputs(op, n, 5, 7)
            assert len(xs) == n and all(x.dtype == F32 and x.shape == (5, 7) and M.normal_or_zero(x) for x in xs)
    assert not M.normal_or_zero(F32(1e-40)) and not M.normal_or_zero(np.inf) and M.normal_or_zero(F32(0))
    a, b = M.special_inputs()
    mx, mn = M.ref_f32("max", [a, b])[0], M.ref_f32("min", [a, b])[0]
    assert np.isnan(mx[4:9]).all() and np.isnan(mn[4:9]).all()               # NaN in either position, beside inf too
    assert mx[:4].tolist() == [np.inf, np.inf, 1, 1] and mn[:4].tolist() == [1, 1, -np.inf, -np.inf] and mx[9] == mn[9] == 2.5
    assert (a[0, M.ZERO_PAIRS] == 0).all() and (np.signbit(a[0, M.ZERO_PAIRS]) != np.signbit(b[0, M.ZERO_PAIRS])).all()
    z, nz = np.array([0.0], dtype=F32), np.array([-0.0], dtype=F32)
    assert not M.same_f32(z, nz) and M.same_f32(z, nz, slice(0, 1)) and M.same_f32(np.array([np.nan], dtype=F32), -np.array([np.nan], dtype=F32))
    assert not M.same_f32(np.array([1.0], dtype=F32), np.array([np.nextafter(F32(1), F32(2))], dtype=F32), slice(0, 1))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_the_extension_header_and_the_exports():
    hdr = open(os.path.join(ROOT, "include", "qnn_abi_merge.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(qnn_[a-z0-9_]+)\s*\(", code))) == sorted(_abi.EXPORTS_MERGE)
    assert _abi.EXPORTS_MERGE == ["qnn_merge_out_store", "qnn_merge_forward"]
    assert re.search(r"#define QNN_MERGE_MAX\s+8\b", hdr) and _abi.MERGE_MAX == 8
    for name, value in (("ADD", 0), ("SUB", 1), ("MUL", 2), ("AVG", 3), ("MAXIMUM", 4), ("MINIMUM", 5)):
        assert re.search(r"\bQNN_MERGE_%s = %d\b" % (name, value), code) and getattr(_abi, "MERGE_" + name) == value
    others = _abi.EXPORTS + _abi.EXPORTS_QACT + _abi.EXPORTS_DILATION + _abi.EXPORTS_MAXACT + _abi.EXPORTS_POOL + \
        _abi.EXPORTS_SCALED + _abi.EXPORTS_CONCAT + _abi.EXPORTS_SPATIAL + _abi.EXPORTS_DEPTHWISE + _abi.EXPORTS_TCONV + \
        _abi.EXPORTS_GCONV
    assert not set(_abi.EXPORTS_MERGE) & set(others)
    assert len(_abi.EXPORTS) == 29 and "qnn_merge" not in open(os.path.join(ROOT, "include", "qnn_abi.h")).read()
    lib = ctypes.CDLL(_abi.lib_path())
    assert all(hasattr(lib, n) for n in _abi.EXPORTS_MERGE)
    lib = _abi.load()
    assert lib.qnn_version() == 4
    ci, vp = ctypes.c_int, ctypes.c_void_p
    assert lib.qnn_merge_out_store.argtypes == [ci, ci]
    assert lib.qnn_merge_forward.argtypes == [ctypes.POINTER(_abi.Merge), ci, ci, ctypes.c_size_t, ci, ci, vp, vp]


def test_ctypes_mirror_matches_the_header_layout(tmp_path):
    """Size and every field offset of _abi.Merge against what the C compiler makes of include/qnn_abi_merge.h."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['printf("size %zu\\n", sizeof(qnn_merge_t));']
    for fname, _ in _abi.Merge._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(qnn_merge_t, %s));' % (fname, fname))
    lines.append('printf("ops %d %d %d %d %d %d\\n", QNN_MERGE_ADD, QNN_MERGE_SUB, QNN_MERGE_MUL, QNN_MERGE_AVG, '
                 'QNN_MERGE_MAXIMUM, QNN_MERGE_MINIMUM);')
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"qnn_abi_merge.h\"\nint main(void) {\n%s\nreturn 0; }\n"
                   % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(ln.split(None, 1) for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(_abi.Merge) == 4 + 4 + 8 * 8
    for fname, _ in _abi.Merge._fields_:
        assert int(out[fname]) == getattr(_abi.Merge, fname).offset, fname
    assert [int(v) for v in out["ops"].split()] == [_abi.MERGE_OPS[op] for op in M.OPS] == list(range(6))
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qnn_abi_merge.h")).read(), flags=re.S)
    body = re.search(r"typedef struct qnn_merge \{([^{}]*)\} qnn_merge_t;", code).group(1)
    fields = [re.sub(r"\[.*\]", "", d.split()[-1].lstrip("*")) for d in body.split(";") if d.strip()]
    assert fields == [n for n, _ in _abi.Merge._fields_] == ["n", "op", "x"]


def test_out_store_states_the_table():
    lib = _abi.load()
    for op in M.OPS:
        for kind in M.STORE:
            assert lib.qnn_merge_out_store(M.OP_CODE[op], M.STORE[kind]) == M.STORE[M.out_kind(op, kind)], (op, kind)
            assert _abi.merge_out_store(op, M.STORE[kind]) == M.STORE[M.out_kind(op, kind)]
    for op, store in ((-1, 0), (6, 0), (0, 3), (0, _abi.STORE_U8), (4, _abi.STORE_F32_IMAGE), (0, -1)):
        assert lib.qnn_merge_out_store(op, store) == EINVAL and b"qnn_merge_out_store" in lib.qnn_last_error()
    with pytest.raises(_abi.QnnError):
        _abi.merge_out_store("dot", 0)


def _desc(n=2, op=4, ptrs=None):
    d = _abi.Merge()
    d.n, d.op = n, op
    for i in range(min(max(n, 0), 8)):
        d.x[i] = ((1 << 40) + (i << 32)) if ptrs is None else ptrs[i]
    return d


def test_forward_refuses_bad_arguments_before_any_device_call():
    """No GPU here: every answer below is given before the first HIP call.  The pointers are never read."""
    lib = _abi.load()
    y = ctypes.c_void_p(1 << 50)
    F, B, T2, I4, I8 = _abi.STORE_F32, _abi.STORE_BIN, _abi.STORE_T2, _abi.STORE_I4, _abi.STORE_I8
    ADD, SUB, MUL, AVG, MAX, MIN = range(6)

    def fwd(n=2, op=MAX, store=I4, bits=4, pixels=7, channels=5, out="table", yp=y, ptrs=None, d="make"):
        if d == "make":
            d = _desc(n, op, ptrs)
        if out == "table":
            out = max(lib.qnn_merge_out_store(op, store), 0)
        rc = lib.qnn_merge_forward(ctypes.byref(d) if d is not None else None, store, bits, pixels, channels, out, yp, None)
        if rc != 0:
            assert b"qnn_merge_forward" in lib.qnn_last_error(), lib.qnn_last_error()        # every message names the entry
        return rc

    assert fwd(d=None) == EINVAL                                               # null descriptor
    assert fwd(n=1) == EINVAL and fwd(n=9) == EINVAL and fwd(n=0) == EINVAL and fwd(n=-1) == EINVAL
    assert fwd(op=-1, out=I4) == EINVAL and fwd(op=6, out=I4) == EINVAL
    assert fwd(op=SUB, n=3) == EINVAL and fwd(op=SUB, n=8) == EINVAL and b"subtraction" in lib.qnn_last_error()
    for store in (3, 5, _abi.STORE_U8, _abi.STORE_F32_IMAGE, _abi.STORE_F32_UNIT, -1):
        assert fwd(store=store, out=store) == EINVAL, store
    assert fwd(bits=5) == EINVAL and fwd(bits=0) == EINVAL and fwd(store=I8, bits=9) == EINVAL
    assert fwd(channels=0) == EINVAL and fwd(channels=-3) == EINVAL
    # out_store is the table's
    assert fwd(out=F) == EINVAL and b"out_store" in lib.qnn_last_error()
    assert fwd(op=ADD, out=I4) == EINVAL and fwd(op=MUL, out=I4) == EINVAL and fwd(op=MUL, store=B, out=F) == EINVAL
    assert fwd(store=F, bits=0, out=I4) == EINVAL
    assert fwd(yp=None) == EINVAL and fwd(ptrs=[1 << 40, 0]) == EINVAL         # null pointers
    assert b"null" in lib.qnn_last_error()
    # y overlapping an input: the same address, an input that begins inside y, y beginning inside an input
    assert fwd(yp=ctypes.c_void_p(1 << 40)) == EINVAL and b"overlap" in lib.qnn_last_error()
    assert fwd(ptrs=[1 << 40, (1 << 50) + 4]) == EINVAL and b"overlap" in lib.qnn_last_error()
    assert fwd(ptrs=[(1 << 50) - 4 * 7 + 4, 1 << 40]) == EINVAL
    assert fwd(op=ADD, ptrs=[(1 << 50) + 4 * 7 * 5 - 4, 1 << 40]) == EINVAL    # float32 out: y is 7 x 5 values long
    # pixels x (words or values of a row) >= 2^31
    assert fwd(channels=8, pixels=1 << 31) == EUNSUPPORTED
    assert fwd(op=ADD, channels=8, pixels=1 << 28) == EUNSUPPORTED             # 2^31 float32 values out of 2^28 words
    assert fwd(store=F, bits=0, channels=2, pixels=1 << 30) == EUNSUPPORTED
    assert fwd(store=T2, channels=32, pixels=1 << 30) == EUNSUPPORTED
    assert fwd(store=B, channels=3, pixels=(1 << 31) + 5) == EUNSUPPORTED
    # no pixels: fine, nothing is launched and the pointers may be null -- but only with valid arguments
    null = _desc(2, MAX, [0, 0])
    for store, bits in ((F, 0), (B, 1), (T2, 1), (I4, 4), (I4, 2), (I8, 8)):
        assert fwd(store=store, bits=bits, pixels=0) == 0
        assert fwd(store=store, bits=bits, pixels=0, yp=None, d=null) == 0
    assert fwd(pixels=0, n=8) == 0 and fwd(pixels=0, op=AVG, n=7) == 0
    assert fwd(pixels=0, bits=7) == EINVAL and fwd(pixels=0, store=3, out=3) == EINVAL and fwd(pixels=0, n=1) == EINVAL
    assert fwd(pixels=0, channels=0) == EINVAL and fwd(pixels=0, out=F) == EINVAL


def test_the_binding_refuses_before_the_library():
    a, b = torch.zeros(7, 3), torch.zeros(7, 3)
    with pytest.raises(_abi.QnnError, match="no CPU path"):
        _abi.merge([a, b], "add", _abi.STORE_F32, 0, 7, 3)                     # CPU tensors
    with pytest.raises(_abi.QnnError, match="contiguous int32 CUDA"):
        _abi.merge([a.int(), b.int()], "max", _abi.STORE_I4, 4, 7, 3)
    with pytest.raises(_abi.QnnError, match="9 inputs"):
        _abi.merge([a] * 9, "add", _abi.STORE_F32, 0, 7, 3)
    with pytest.raises(_abi.QnnError, match="1 inputs"):
        _abi.merge([a], "add", _abi.STORE_F32, 0, 7, 3)
    with pytest.raises(_abi.QnnError, match="exactly 2"):
        _abi.merge([a, b, a], "sub", _abi.STORE_F32, 0, 7, 3)
    with pytest.raises(_abi.QnnError, match="fn="):
        _abi.merge([a, b], "dot", _abi.STORE_F32, 0, 7, 3)
    with pytest.raises(_abi.QnnError):
        _abi.merge([a, b], "add", _abi.STORE_U8, 0, 7, 3)


# ---- the layer classes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", M.OPS)
def test_layer_class(fn):
    cls = LAYERS[fn]
    assert cls.__name__ in qnn_amd.__all__ and cls.fn == fn
    l = cls()
    assert l.name == cls.__name__.lower() and l.get_config() == {"name": cls.__name__.lower(), "trainable": True}
    cfg = cls(name="m", trainable=True).get_config()
    assert cfg == {"name": "m", "trainable": True} and cls.from_config(cfg).get_config() == cfg
    with pytest.raises(TypeError):
        cls(axis=1)
    assert l.compute_output_shape([(None, 8, 8, 12), (None, 8, 8, 12)]) == (None, 8, 8, 12)
    assert l.compute_output_shape([(4, 10), (4, 10)]) == (4, 10)
    a = torch.zeros(2, 4, 4, 3)
    with pytest.raises(ValueError, match="should be called on a list of inputs"):
        l(a)
    for bad in ([a], []):
        with pytest.raises(ValueError, match="should be called on a list of at least 2 inputs. Got %d inputs" % len(bad)):
            l(bad)
    if fn == "sub":
        with pytest.raises(ValueError, match="A `Subtract` layer should be called on exactly 2 inputs"):
            l([a, a, a])
        with pytest.raises(ValueError, match="exactly 2 inputs"):
            l.compute_output_shape([(2, 3)] * 3)
    else:
        assert l.compute_output_shape([(2, 3)] * 8) == (2, 3)
        with pytest.raises(_abi.QnnError, match="9 inputs"):
            l([a] * 9)
    # Keras would broadcast these: refused, naming the shapes
    for other in (torch.zeros(2, 4, 4, 1), torch.zeros(1, 4, 4, 3), torch.zeros(4, 4, 3), torch.zeros(2, 48)):
        with pytest.raises(_abi.QnnError, match=re.escape(str(tuple(other.shape)))):
            l([a, other])
    with pytest.raises(_abi.QnnError, match="no CPU path"):
        l([a, a])                                                              # CPU tensors: there is no CPU path


# ---- the importer ---------------------------------------------------------------------------------------------------------
def _npz(tmp_path, cls, inbound):
    layer = lambda c, name, ib, **cfg: {"class_name": c, "name": name, "config": dict(cfg, name=name),      # noqa: E731
                                        "inbound_nodes": [[[i, 0, 0, {}] for i in ib]] if ib else []}
    pool = dict(pool_size=[2, 2], strides=[2, 2], padding="valid", data_format="channels_last")
    cfg = {"class_name": "Model", "config": {"layers": [
        layer("InputLayer", "in", []),
        layer("MaxPooling2D", "p", ["in"], **pool),
        layer("AveragePooling2D", "q", ["in"], **pool),
        layer(cls, "m", inbound, trainable=True),
        layer("Flatten", "f", ["m"])]}}
    path = tmp_path / ("%s%d.npz" % (cls, len(inbound)))
    np.savez(path, model_config_json=np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8))
    return str(path)


def test_importer_maps_the_merge_layers(tmp_path):
    names = {"Add": "add", "Subtract": "sub", "Multiply": "mul", "Average": "avg", "Maximum": "max", "Minimum": "min"}
    for cls, fn in names.items():
        for inbound in (["p", "q"], ["p", "q", "p"], ["in", "in"]):
            if cls == "Subtract" and len(inbound) != 2:
                with pytest.raises(ValueError, match="3 inbound"):
                    nets.spec_from_keras_npz(_npz(tmp_path, cls, inbound))
                continue
            spec = nets.spec_from_keras_npz(_npz(tmp_path, cls, inbound))
            srcs = ["input" if s == "in" else s for s in inbound]
            if cls == "Add" and len(inbound) == 2:                             # the two-input Add stays the add op it was
                assert spec[2] == {"op": "add", "a": srcs[0], "b": inbound[1], "dst": "m"}        # (as the importer always wrote it)
            else:
                assert spec[2] == {"op": "merge", "fn": fn, "srcs": srcs, "dst": "m"}
            assert spec[3] == {"op": "flatten", "src": "m", "dst": "f"}
    with pytest.raises(ValueError, match="unsupported layer class 'Dot'"):
        nets.spec_from_keras_npz(_npz(tmp_path, "Dot", ["p", "q"]))


# ---- the engines' reading of the op ---------------------------------------------------------------------------------------
def _spec(fn="max", n=2):
    net = C.S.Net(7, hw=(8, 8))
    a0 = net.conv(16, dst="c0")
    net.bn(dst="b0")
    a0 = net.act(dst="a0")
    branches = []
    for i in range(n):
        net.conv(16, src=a0, dst="c%d" % (i + 1))
        net.bn(dst="b%d" % (i + 1))
        branches.append(net.act(dst="a%d" % (i + 1)))
    net.spec.append({"op": "merge", "fn": fn, "srcs": branches, "dst": "m"})
    net.shape["m"] = net.shape[branches[0]]
    net.cur = "m"
    net.conv(16)
    return net.spec


def test_spec_graph_lists_every_source_of_a_merge():
    spec = _spec("avg", 3)
    g = engine._SpecGraph(spec, "cpu")
    i = g.prod["m"]
    assert g.srcs[i] == ["a1", "a2", "a3"] and all(i in g.cons[s] for s in g.srcs[i])
    assert g.cons["a0"] == [g.prod["c1"], g.prod["c2"], g.prod["c3"]] and g.cons["m"] == [i + 1]
    two = [{"op": "merge", "fn": "mul", "srcs": ["input", "input"], "dst": "m"}]
    assert engine._SpecGraph(two, "cpu").srcs == [["input", "input"]]
    # the existing two-input add is read as before
    assert engine._SpecGraph([{"op": "add", "a": "input", "b": "input"}], "cpu").srcs == [["input", "input"]]


@pytest.mark.parametrize("fn", M.OPS)
def test_the_fused_engines_refuse_a_merge_by_name(fn):
    spec = _spec(fn)
    for cls in (engine.FusedModel, engine.ResidualFusedModel):
        with pytest.raises(_abi.NotFusable, match="merge"):
            cls(spec)


def test_the_engine_checks_a_merge_ops_sources():
    for bad, match in (({"op": "merge", "fn": "dot"}, "fn="), ({"op": "merge", "fn": "sub"}, "exactly 2"),
                       ({"op": "merge", "fn": "add"}, "sources")):
        n = 3 if bad["fn"] == "sub" else 9 if bad["fn"] == "add" else 2
        with pytest.raises(ValueError, match=match):
            engine._merge_shape([(2, 3)] * n, bad)
    with pytest.raises(_abi.QnnError, match=r"\(2, 3\).*\(2, 1\)"):
        engine._merge_shape([(2, 3), (2, 1)], {"op": "merge", "fn": "add"})
    assert engine._merge_shape([(2, 8, 8, 3)] * 8, {"op": "merge", "fn": "avg"}) == (2, 8, 8, 3)
