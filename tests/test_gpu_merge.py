"""The merge entry on the GPU (include/qnn_abi_merge.h, csrc/qnn_merge.hip) against the numpy reference of merge_cases.py,
bit for bit, with the kernel name asserted: every op on every store at every channel count, pixel count, code width and
n = 2, 3, 8 of the case table, with the inputs' spare bits set, and with every pointer moved off its 16-byte alignment;
the float32 inf / NaN / equal / +-0 pairs; avg at n = 3, 5, 6, 7 (the cases test_merge_cpu.py proves to tell a division from
a reciprocal); the packed maximum as the input of a convolution; each refusal with the output buffer untouched; no pixels;
the six layer classes.  The checks below run in turn as ONE test, test_the_merge_entry: they share the case tables, and
the suite's list of GPU test ids stays short; every assertion names its case.

The kernel forms (merge_cases.form restates the host's rule; the name qnn_last_kernel() gives is per family).  With the
tensors where torch allocates them (16-byte aligned) the 16-byte form runs:
  merge_f32                     4 channels at every pixel count; 1, 3 and 7 channels at 64 pixels
  merge_bin / _i4 / _i8 / _t2   rows without spare bits whose words divide by 4: BIN 128, I4 64, I8 16 channels at every
                                pixel count; BIN 32, I4 8, I8 4 and T2 32 channels at 64 pixels
  merge_*_f32                   channels that divide by 4: BIN 32, 128; I4 8, 12, 64; I8 4, 16; T2 32
and the 4-byte form every other case of the table (the ragged rows among them: BIN 3 and 33, I4 5 and 12, I8 3 and 6, T2 3
and 33 channels) and every call with moved pointers, whatever its shape."""
import ctypes

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi, engine

import merge_cases as M

pytestmark = pytest.mark.gpu
F32 = np.float32
FILL = 0x5A5A5A5A
ENTRIES = _abi.EXPORTS_MERGE             # read at import: without the entries, the op and the classes nothing below means anything
LAYERS = {"add": qnn_amd.Add, "sub": qnn_amd.Subtract, "mul": qnn_amd.Multiply, "avg": qnn_amd.Average,
          "max": qnn_amd.Maximum, "min": qnn_amd.Minimum}


@pytest.fixture(scope="module", autouse=True)
def _drop_the_case_tables():
    """The cached codes and operands (about 100 MB) are shared by the tests of this file and freed behind the last one."""
    yield
    M.codes.cache_clear()
    M.f32_inputs.cache_clear()


def dev(a):
    a = np.array(a, order="C")               # a writable copy: the case tables are read-only
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host(t):
    torch.cuda.synchronize()
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def off_by_a_word(a):
    """A device copy of `a` whose address is 4 bytes past a 16-byte boundary, and the buffer around it."""
    t = dev(a)
    buf = torch.full((t.numel() + 4,), FILL, dtype=torch.int32, device="cuda").view(t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v, buf


def raw(xs, op, kind, bits, pixels, channels, y, out_store=None, n=None):
    """qnn_merge_forward on the caller's own output tensor: the status."""
    d = _abi.Merge()
    d.n, d.op = len(xs) if n is None else n, M.OP_CODE[op] if isinstance(op, str) else op
    for i, t in enumerate(xs[:8]):
        d.x[i] = t.data_ptr() if t is not None else 0
    if out_store is None:
        out_store = M.STORE[M.out_kind(op, kind)]
    return _abi.load().qnn_merge_forward(ctypes.byref(d), M.STORE[kind], bits, pixels, channels, out_store,
                                         _abi.ptr(y), _abi.stream_ptr())


def kernel_name(op, kind):
    return "merge_f32" if kind == "f32" else "merge_" + kind + ("" if M.out_kind(op, kind) == kind else "_f32")


def case(op, kind, bits, pixels, c, n):
    """(inputs as stored: words with every spare bit set, or float32 values; the expected output as stored; the spare
    bits of an output row)."""
    if kind == "f32":
        xs = M.f32_inputs(op, n, pixels, c)
        return list(xs), M.ref_f32(op, xs), None
    ks = [M.codes(kind, bits, pixels, c, i) for i in range(n)]
    ws = [M.encode(k, kind) | M.spare(kind, c) for k in ks]
    if kind == "t2":                     # sign bits under clear mask bits as well: they never reach the result
        for w in ws:
            w[:, 1::2] |= ~w[:, 0::2]
        assert all(np.array_equal(M.decode(w, kind, c), k) for w, k in zip(ws, ks))
    if M.out_kind(op, kind) == kind:
        return ws, M.encode(M.ref_codes(op, kind, bits, ks), kind), M.spare(kind, c)
    return ws, M.ref_f32(op, [M.values(k, kind, bits) for k in ks]), None


def check(got, want, msg):
    if want.dtype == np.uint32:
        np.testing.assert_array_equal(got, want, err_msg=msg)
    else:
        assert got.dtype == F32 and M.same_f32(got, want), msg


ALL = [(op, kind) for kind in ("f32", "bin", "i4", "i8", "t2") for op in M.OPS]


def check_every_op_on_every_store(op, kind):
    store, name = M.STORE[kind], kernel_name(op, kind)
    for c in M.CHANNELS[kind]:
        for pixels in M.PIXELS:
            for bits in M.BITS[kind]:
                for n in M.ns_of(op):
                    xs, want, sp = case(op, kind, bits, pixels, c, n)
                    msg = "%s %s channels=%d pixels=%d bits=%d n=%d" % (op, kind, c, pixels, bits, n)
                    y, out_store = _abi.merge([dev(x) for x in xs], op, store, bits, pixels, c)
                    assert _abi.last_kernel() == name and out_store == M.STORE[M.out_kind(op, kind)], msg
                    got = host(y)
                    assert got.shape == want.shape, msg
                    check(got, want, msg)
                    if sp is not None:
                        assert not np.any(got & sp), msg               # the inputs' spare bits were ones
                    if n != 2 and not (n == 8 and pixels == 2051):
                        continue                                       # (moved pointers: n = 2 everywhere, 8 at the largest)
                    # every pointer one word past a 16-byte boundary: the 4-byte form, the same bits, nothing written around y
                    moved = [off_by_a_word(x) for x in xs]
                    yv, ybuf = off_by_a_word(np.full(want.shape, FILL, dtype=np.uint32))
                    if want.dtype != np.uint32:
                        yv = yv.view(torch.float32)
                    assert raw([v for v, _ in moved], op, kind, bits, pixels, c, yv) == 0, msg
                    assert _abi.last_kernel() == name
                    check(host(yv), want, "moved pointers " + msg)
                    edge = host(ybuf)
                    assert edge[0] == FILL and np.all(edge[1 + want.size:] == FILL), msg


def check_avg_divides_by_n(n):
    """One correctly rounded division by float32(n), not a multiplication by the reciprocal: every case holds an element
    where the two differ (test_merge_cpu.py)."""
    for c in M.CHANNELS["f32"]:
        xs = M.f32_inputs("avg", n, 64, c)
        y, _ = _abi.merge([dev(x) for x in xs], "avg", _abi.STORE_F32, 0, 64, c)
        assert _abi.last_kernel() == "merge_f32"
        want = M.ref_f32("avg", xs)
        assert np.any(want != M.ref_f32("add", xs) * (F32(1) / F32(n)))
        assert M.same_f32(host(y), want), (n, c)
    # on codes: the exact integer sum, then the same division
    for kind, bits, c in (("i4", 4, 12), ("i8", 8, 6), ("bin", 1, 33), ("t2", 1, 32)):
        ks = [M.codes(kind, bits, 64, c, i) for i in range(n)]
        y, out_store = _abi.merge([dev(M.encode(k, kind)) for k in ks], "avg", M.STORE[kind], bits, 64, c)
        assert _abi.last_kernel() == "merge_%s_f32" % kind and out_store == _abi.STORE_F32
        assert M.same_f32(host(y), M.ref_f32("avg", [M.values(k, kind, bits) for k in ks])), (kind, n)


def check_float32_nan_inf_equal_values_and_zero_pairs(op):
    for n in (2, 3):
        xs = M.special_inputs(n)
        want = M.ref_f32(op, xs)
        assert np.isnan(want).sum() == 5
        for form in ("as it is", "moved"):
            if form == "moved":
                ts = [off_by_a_word(x)[0] for x in xs]
                y = off_by_a_word(np.zeros(want.shape, dtype=F32))[0]
                assert raw(ts, op, "f32", 0, 1, want.shape[1], y) == 0
            else:
                y, _ = _abi.merge([dev(x) for x in xs], op, _abi.STORE_F32, 0, 1, want.shape[1])
            assert _abi.last_kernel() == "merge_f32"
            got = host(y)
            assert M.same_f32(got, want, M.ZERO_PAIRS), (op, n, form, got, want)     # +0 / -0 pairs: by value
            assert np.array_equal(np.isnan(got), np.isnan(want))
    # 16 columns of it: the 16-byte form (14 are not a multiple of 4)
    xs = [np.concatenate([x, x[:, :2]], axis=1) for x in M.special_inputs(2)]
    assert M.form(op, "f32", 16, 1) == 16
    y, _ = _abi.merge([dev(x) for x in xs], op, _abi.STORE_F32, 0, 1, 16)
    assert M.same_f32(host(y)[:, :14], M.ref_f32(op, xs)[:, :14], M.ZERO_PAIRS)


def check_merge_of_packs_is_pack_of_the_merge():
    """The library's own pack / unpack around the entry: max of packed codes == pack of the float32 max, and the float32-out
    forms == the float32 form on the unpacked values."""
    pixels = 35
    for kind, bits, c in (("bin", 1, 33), ("i4", 3, 12), ("i4", 4, 64), ("i8", 8, 6), ("t2", 1, 33)):
        store = M.STORE[kind]
        vals = [M.values(M.codes(kind, bits, pixels, c, 10 + i), kind, bits) for i in range(3)]
        packs = [_abi.pack(dev(v), c, _abi.FN_GRID, bits, store) for v in vals]
        for op in M.OPS:
            xs, ps = (vals[:2], packs[:2]) if op == "sub" else (vals, packs)
            y, out_store = _abi.merge(ps, op, store, bits, pixels, c)
            f, _ = _abi.merge([_abi.unpack(p, pixels, c, store, bits) for p in ps], op, _abi.STORE_F32, 0, pixels, c)
            assert M.same_f32(host(f), M.ref_f32(op, xs))
            if out_store == _abi.STORE_F32:
                assert torch.equal(y, f), (kind, op)
            else:
                assert torch.equal(y, _abi.pack(f, c, _abi.FN_GRID, bits, store)), (kind, op)


def check_the_packed_maximum_feeds_a_convolution(c):
    """conv(max of the packed codes) == conv(float32 max), bit for bit: dyadic operands, every sum exact."""
    N, H, W = 2, 5, 4
    rng = np.random.default_rng(7)
    op = {"op": "conv", "kind": "quantized", "nb": 4, "kernel": (rng.integers(-8, 8, (3, 3, c, 16)) / 8.0).astype(F32), "bias": None}
    vals = [M.values(M.codes("i4", 4, N * H * W, c, 20 + i), "i4", 4) for i in range(2)]
    packs = [_abi.pack(dev(v), c, _abi.FN_GRID, 4, _abi.STORE_I4) for v in vals]
    xp, out_store = _abi.merge(packs, "max", _abi.STORE_I4, 4, N * H * W, c)
    assert _abi.last_kernel() == "merge_i4" and out_store == _abi.STORE_I4
    y_codes = _abi.conv2d(engine._prepack(op, _abi.STORE_I4, "cuda"), xp, _abi.STORE_I4, 4, N, H, W)[0]
    xf, _ = _abi.merge([dev(v) for v in vals], "max", _abi.STORE_F32, 0, N * H * W, c)
    np.testing.assert_array_equal(host(xf), np.maximum(*vals))
    y_f32 = _abi.conv2d(engine._prepack(op, _abi.STORE_F32, "cuda"), xf.reshape(N, H, W, c), _abi.STORE_F32, 0, N, H, W)[0]
    assert y_codes.shape == y_f32.shape == (N, H, W, 16)
    assert torch.equal(y_codes, y_f32) and float(y_f32.abs().max()) > 0


def check_every_refusal_leaves_the_output_untouched():
    EINVAL, EUNSUPPORTED = -1, -2
    pixels, c = 7, 12
    ws = [dev(M.encode(M.codes("i4", 4, pixels, c, i), "i4")) for i in range(8)]
    y = torch.full((pixels, max(M.words("i4", c), c)), FILL, dtype=torch.int32, device="cuda")
    lib = _abi.load()
    I4, F = _abi.STORE_I4, _abi.STORE_F32

    def fwd(xs=ws[:2], op="max", kind="i4", bits=4, px=pixels, ch=c, out=None, n=None, yt=y):
        rc = raw(xs, op, kind, bits, px, ch, yt, out, n)
        torch.cuda.synchronize()
        assert np.all(host(y) == FILL), lib.qnn_last_error()
        return rc

    d_null = lib.qnn_merge_forward(None, I4, 4, pixels, c, I4, _abi.ptr(y), _abi.stream_ptr())
    assert d_null == EINVAL and np.all(host(y) == FILL)
    assert fwd(n=1) == EINVAL and fwd(n=9) == EINVAL and fwd(n=0) == EINVAL
    assert fwd(op=6, out=I4) == EINVAL and fwd(op=-1, out=I4) == EINVAL
    assert fwd(xs=ws[:3], op="sub") == EINVAL
    assert raw(ws[:2], "max", "i4", 4, pixels, c, y, 3) == EINVAL and fwd(out=F) == EINVAL and fwd(op="add", out=I4) == EINVAL
    for store in (3, 5, _abi.STORE_U8, _abi.STORE_F32_IMAGE):
        d = _abi.Merge()
        d.n, d.op, d.x[0], d.x[1] = 2, 4, ws[0].data_ptr(), ws[1].data_ptr()
        assert lib.qnn_merge_forward(ctypes.byref(d), store, 4, pixels, c, store, _abi.ptr(y), _abi.stream_ptr()) == EINVAL
    assert fwd(bits=5) == EINVAL and fwd(bits=0) == EINVAL and fwd(kind="i8", bits=9) == EINVAL
    assert fwd(ch=0) == EINVAL and fwd(ch=-1) == EINVAL
    assert fwd(xs=[ws[0], None]) == EINVAL and fwd(yt=None) == EINVAL
    # y overlapping an input: y itself, and y beginning inside an input
    assert fwd(xs=[ws[0], y]) == EINVAL and b"overlap" in lib.qnn_last_error()
    assert fwd(xs=[ws[0], y.view(-1)[4:]]) == EINVAL and fwd(xs=[y.view(-1)[4:], ws[0]], op="add") == EINVAL
    assert fwd(px=1 << 31, ch=8) == EUNSUPPORTED and fwd(op="add", px=1 << 28, ch=8) == EUNSUPPORTED
    assert fwd(kind="f32", bits=0, px=1 << 30, ch=2) == EUNSUPPORTED
    assert np.all(host(y) == FILL)
    # and the call those were variations of is a valid one
    assert raw(ws[:2], "max", "i4", 4, pixels, c, y) == 0 and not np.all(host(y) == FILL)


def check_no_pixels():
    y = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
    for op, kind in ALL:
        for bits in M.BITS[kind][-1:]:
            assert raw([y, y], op, kind, bits, 0, 5, y) == 0               # nothing is launched: the pointers are not looked at
            assert raw([None, None], op, kind, bits, 0, 5, None) == 0
    assert raw([y, y], "max", "i4", 9, 0, 5, y) == -1 and raw([y], "max", "i4", 4, 0, 5, y) == -1
    empty = torch.empty((0, 5), dtype=torch.float32, device="cuda")
    out, out_store = _abi.merge([empty, empty], "add", _abi.STORE_F32, 0, 0, 5)
    assert out.shape == (0, 5) and out_store == _abi.STORE_F32
    assert np.all(host(y) == FILL)


def check_the_layer_classes(fn):
    layer = LAYERS[fn]()
    for n in M.ns_of(fn):
        xs = [x.reshape(2, 7, 5, 12) for x in M.f32_inputs(fn, n, 70, 12, seed=3)]
        y = layer([dev(x) for x in xs])
        assert _abi.last_kernel() == "merge_f32" and y.shape == (2, 7, 5, 12) and y.dtype == torch.float32
        assert M.same_f32(host(y), M.ref_f32(fn, xs)), (fn, n)
    flat = M.f32_inputs(fn, 2, 5, 7, seed=4)
    assert M.same_f32(host(layer([dev(x) for x in flat])), M.ref_f32(fn, flat))
    a = dev(flat[0])
    with pytest.raises(ValueError, match="at least 2 inputs"):
        layer([a])
    with pytest.raises(_abi.QnnError, match=r"\(5, 7\).*\(5, 1\)"):
        layer([a, a[:, :1]])
    with pytest.raises(_abi.QnnError, match="no CPU path"):
        layer([a, a.cpu()])
    if fn == "sub":
        with pytest.raises(ValueError, match="exactly 2 inputs"):
            layer([a, a, a])


def test_the_merge_entry():
    for op, kind in ALL:
        check_every_op_on_every_store(op, kind)
    for n in M.AVG_NS:
        check_avg_divides_by_n(n)
    for op in ("max", "min"):
        check_float32_nan_inf_equal_values_and_zero_pairs(op)
    check_merge_of_packs_is_pack_of_the_merge()
    for c in (12, 16):
        check_the_packed_maximum_feeds_a_convolution(c)
    check_every_refusal_leaves_the_output_untouched()
    check_no_pixels()
    for fn in M.OPS:
        check_the_layer_classes(fn)
