"""Everything behind the convolutions, at its edges, on the GPU: qnn_dense_forward (the dense kernels and the fall-through
into the convolution routes at H = W = 1), qnn_avgpool_packed_f32, qnn_softmax_f32, qnn_pack_f32 / qnn_unpack_f32 and the
elementwise activations, each against the references of tail_cases.py (integer / float64 numpy, proven equal to the oracle
by test_tail_cases_cpu.py).

Every output buffer is allocated with one guard row before and after the region handed to the library and pre-filled (a
NaN pattern for float32, 0x5a5a5a5a for packed words): after the call the guards must be untouched and the region must hold
no fill value, so a store outside the region or a row that was never written is an assertion here.  The tests only compare
results."""
import ctypes

import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine
from oracle import qnn_oracle as O
import tail_cases as T

pytestmark = pytest.mark.gpu
F32 = np.float32
NAN_FILL = 0x7fc5a5a5                      # a quiet NaN with a recognisable payload
FN = {"none": _abi.FN_NONE, "binary_tanh": _abi.FN_BINARY_TANH, "quantized_tanh": _abi.FN_QUANTIZED_TANH}
WKIND = {"binary": _abi.W_BINARY, "ternary": _abi.W_TERNARY, "quantized": _abi.W_QUANT, "float": _abi.W_FLOAT}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def dev_words(w):
    return dev(np.ascontiguousarray(w).view(np.int32))


class Guarded:
    """`rows` x `width` 4-byte elements with a guard row on either side, all pre-filled."""

    def __init__(self, rows, width, packed):
        self.rows, self.width, self.packed = rows, width, packed
        self.fill = T.PACKED_FILL if packed else NAN_FILL
        self.full = torch.full((rows + 2, width), self.fill, dtype=torch.int32, device="cuda")
        self.ptr = ctypes.c_void_p(self.full.data_ptr() + 4 * width)

    def region(self):
        r = self.full[1:self.rows + 1]
        return r if self.packed else r.view(torch.float32)

    def check(self, what):
        torch.cuda.synchronize()
        f = self.full
        assert bool((f[0] == self.fill).all()) and bool((f[-1] == self.fill).all()), "a guard row was written: " + what
        r = f[1:self.rows + 1]
        if self.packed:
            missing = int((r == self.fill).sum())
        else:
            missing = int(torch.isnan(r.view(torch.float32)).sum())
        assert missing == 0, "%d elements of the output were never written (or hold NaN): %s" % (missing, what)


def one_more_row(a):
    """A device copy with a spare row at the end: an N = 0 input still has a non-null pointer."""
    t = torch.zeros((a.shape[0] + 1,) + a.shape[1:], dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    if a.shape[0]:
        t[:a.shape[0]] = dev(a)
    return t


# ---------------------------------------------------------------------------------------------------------------------
# dense
# ---------------------------------------------------------------------------------------------------------------------
class DenseCall:
    """A case's weights, epilogue constants and input on the device."""

    def __init__(self, c, d):
        self.c, self.d = c, d
        s = c["x_store"]
        bias = dev(d["bias"]) if d["bias"] is not None else None
        self.w = _abi.Weights(WKIND[c["wkind"]], int(c["wbits"]) if c["wkind"] == "quantized" else 1, 1.0, dev(d["kernel"]),
                              bias, 1, True, s)
        self.inv = self.shift = None
        if d["bn"] is not None:
            self.inv, self.shift = (dev(a) for a in engine.bn_constants(d["bn"]))
        self.res = dev(d["res"]) if d["res"] is not None else None
        self.x = one_more_row(d["x"] if s == T.STORE_F32 else T.pack_words(d["codes"], s).view(np.int32))

    def run(self, x=None, N=None):
        """float32 (N, units) result; a packed output is unpacked with qnn_unpack_f32."""
        c = self.c
        N = c["N"] if N is None else N
        x = self.x if x is None else x
        packed = c["out_store"] != T.STORE_F32
        out = Guarded(N, T.words(c["out_store"], c["units"]) if packed else c["units"], packed)
        kw = dict(res=self.res, res_store=_abi.STORE_F32, res_bits=0, post_scale=self.d["post_scale"]) if self.res is not None else {}
        epi = _abi.make_epilogue(self.inv, self.shift, FN[c["fn"]], c["act_bits"], 1, c["out_store"], **kw)
        _abi.check(_abi.load().qnn_dense_forward(self.w.handle, _abi.ptr(x), c["x_store"], c["x_bits"], N, ctypes.byref(epi),
                                                 out.ptr, _abi.stream_ptr()), "qnn_dense_forward")
        self.kernel = _abi.last_kernel() if N else "(N = 0: nothing launched)"
        out.check("%s kernel=%s" % (c["id"], self.kernel))
        if not packed:
            return out.region()
        if N == 0:
            return torch.empty((0, c["units"]), dtype=torch.float32, device="cuda")
        nb = c["act_bits"] if c["fn"] == "quantized_tanh" else 1
        return _abi.unpack(out.region().contiguous(), N, c["units"], c["out_store"], nb)


DENSE = T.dense_cases()
GRID_DENSE = [c for c in DENSE if c["x_store"] != T.STORE_F32 or c["xkind"] == "grid"]
REAL_DENSE = [c for c in DENSE if c["x_store"] == T.STORE_F32 and c["xkind"] != "grid"]


@pytest.mark.parametrize("c", GRID_DENSE, ids=[c["id"] for c in GRID_DENSE])
def test_dense_bit_exact(c):
    """Packed inputs and grid-valued float32 inputs: every product and partial sum is exact, so the result is determined
    to the last bit: equal to the int64 reference under both kernel-family preferences, on whatever kernel takes the call;
    the rows written for a route boundary also assert the kernel family they were written for."""
    d = T.dense_inputs(c)
    want = T.dense_reference(c, d)
    call = DenseCall(c, d)
    try:
        for impl in (_abi.IMPL_AUTO, _abi.IMPL_VALU):
            _abi.set_conv_impl(impl)
            got = host(call.run())
            msg = "%s (%s) impl=%d kernel=%s" % (c["id"], c["why"], impl, call.kernel)
            assert got.shape == want.shape, msg
            np.testing.assert_array_equal(got, want, err_msg=msg)
            if c["boundary"] and c["N"]:
                family = "dense" if call.kernel.startswith("dense_") else "conv"
                assert family == T.dense_family(c), msg + ": expected a %s kernel (%s)" % (T.dense_family(c), T.dense_branch(c))
    finally:
        _abi.set_conv_impl(_abi.IMPL_AUTO)


@pytest.mark.parametrize("c", REAL_DENSE, ids=[c["id"] for c in REAL_DENSE])
def test_dense_f32_correctly_rounded(c):
    """float32 inputs off the grid (unit normal, and built to cancel): |got - f32(s)| <= ulp32(s) + K * 2^-53 * sum |x w|
    with s the float64 dot product -- one rounding to float32 plus the worst-case error of K float64 additions in any
    order.  No bias, BN or activation on these rows."""
    d = T.dense_inputs(c)
    s, bound = T.dense_f32_bound(c, d)
    call = DenseCall(c, d)
    got = host(call.run()).astype(np.float64)
    assert call.kernel == "dense_f32", call.kernel
    assert d["bias"] is None and d["bn"] is None and c["fn"] == "none"
    want = s.astype(F32)
    ratio = float((np.abs(got - want.astype(np.float64)) / bound).max())
    assert ratio <= 1.0, "%s kernel=%s: max |got - f32(s)| / bound = %.3g" % (c["id"], call.kernel, ratio)


@pytest.mark.parametrize("form,K", [("split", 1024), ("up16", 96)])
def test_dense_batch_independence_at_4096(form, K):
    """Rows of a shuffled batch equal the shuffled rows, and rows 100..136 run alone equal the same rows of the full call."""
    c = T._case(T.STORE_I4, 4, "quantized", 4, 4096, K, 10, bn="pos", seed=77 + K)
    c["id"] = "batch-independence-" + form
    assert T.dense_branch(c) == form
    d = T.dense_inputs(c)
    call = DenseCall(c, d)
    y = call.run().clone()
    assert call.kernel == "dense_i4"
    np.testing.assert_array_equal(host(y), T.dense_reference(c, d))
    perm = torch.randperm(4096, generator=torch.Generator().manual_seed(3)).cuda()
    xs = call.x.clone()
    xs[:4096] = call.x[:4096][perm]
    assert torch.equal(call.run(x=xs), y[perm])
    part = call.x[100:138].clone()              # rows 100..136 and the spare row
    assert torch.equal(call.run(x=part, N=37), y[100:137])


# ---------------------------------------------------------------------------------------------------------------------
# average pool
# ---------------------------------------------------------------------------------------------------------------------
AVGPOOL = T.avgpool_cases()


@pytest.mark.parametrize("c", AVGPOOL, ids=[c["id"] for c in AVGPOOL])
def test_avgpool_bit_exact(c):
    """Exact window sums of the codes and one float32 division: equal to the float64 / integer reference and to the
    oracle's AveragePooling2D, on the wave kernel, one condition short of it, and where the generic kernel's grid-stride
    loop runs more than once."""
    codes = T.avgpool_codes(c)
    N, H, W, C, size = c["N"], c["H"], c["W"], c["C"], c["size"]
    want = T.avgpool_reference(c, codes)
    xp = dev_words(T.pack_words(codes.reshape(-1, C), c["store"]))
    Ho, Wo = H // size, W // size
    out = Guarded(N * Ho * Wo, C, False)
    _abi.check(_abi.load().qnn_avgpool_packed_f32(_abi.ptr(xp), c["store"], c["bits"], N, H, W, C, size, out.ptr,
                                                  _abi.stream_ptr()), "qnn_avgpool_packed_f32")
    msg = "%s (%s) wave=%s" % (c["id"], c["why"], T.avgpool_wave(c))
    out.check(msg)
    got = host(out.region()).reshape(N, Ho, Wo, C)
    np.testing.assert_array_equal(got, want, err_msg=msg)
    x = (codes.astype(F32) * F32(T.code_scale(c["store"], c["bits"]))).astype(F32)
    np.testing.assert_array_equal(got, O.avgpool2d(x, size), err_msg=msg)


# ---------------------------------------------------------------------------------------------------------------------
# softmax
# ---------------------------------------------------------------------------------------------------------------------
def softmax_ulps(got, want):
    """|got - want| in units of ulp32(want)."""
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / T.ulp32(want)


@pytest.mark.parametrize("rows", T.SOFTMAX_ROWS)
@pytest.mark.parametrize("cols", T.SOFTMAX_COLS)
def test_softmax_within_one_ulp_of_the_float64_definition(rows, cols):
    """qnn_softmax_f32 against the float64 definition rounded once, RELATIVE: |got - want| <= ulp32(want) per element, small
    probabilities and float32 denormals included (an absolute tolerance would let every probability below it be returned
    as 0).  One ulp and not zero: the device's float64 exp may differ from numpy's in the last float64 bit, which can move a
    float32 rounding by one ulp and no more.  Rows sum to 1 within cols * 2^-24.  Finite logits only: non-finite logits are
    out of scope."""
    for c in T.softmax_cases():
        if c["rows"] != rows or c["cols"] != cols:
            continue
        x = T.softmax_logits(c)
        want = T.softmax_reference(x)
        out = Guarded(rows, cols, False)
        xd = dev(x)
        _abi.check(_abi.load().qnn_softmax_f32(_abi.ptr(xd), out.ptr, rows, cols, _abi.stream_ptr()), "qnn_softmax_f32")
        out.check(c["id"])
        got = host(out.region())
        u = softmax_ulps(got, want)
        hist = np.bincount(np.minimum(np.ceil(u).astype(np.int64), 9).reshape(-1), minlength=10)
        print("softmax %s: max %.3f ulp, elements by ceil(ulps) 0..9+: %s" % (c["id"], u.max(), hist.tolist()))
        assert u.max() <= 1.0, "%s: max error %.3f ulp32; elements by ceil(ulps) 0..9+: %s" % (c["id"], u.max(), hist.tolist())
        sums = got.astype(np.float64).sum(-1)
        assert np.abs(sums - 1.0).max() <= cols * 2.0 ** -24, "%s: row sum off by %.3g" % (c["id"], np.abs(sums - 1.0).max())
        _abi.softmax(xd, out=xd)                                            # x == y is allowed
        np.testing.assert_array_equal(host(xd), got, err_msg=c["id"] + " in place")


# ---------------------------------------------------------------------------------------------------------------------
# pack / unpack
# ---------------------------------------------------------------------------------------------------------------------
def _pack_into(xd, pixels, C, fn, nb, store, what):
    out = Guarded(pixels, T.words(store, C), True)
    _abi.check(_abi.load().qnn_pack_f32(_abi.ptr(xd), out.ptr, pixels, C, fn, nb, store, _abi.stream_ptr()), "qnn_pack_f32")
    out.check(what)
    return host(out.region()).view(np.uint32)


@pytest.mark.parametrize("pixels", T.PACK_PIXELS)
@pytest.mark.parametrize("store,bits", T.PACK_FORMATS, ids=["%s%d" % (T.STORE_NAME[s], b) for s, b in T.PACK_FORMATS])
def test_pack_and_unpack_against_the_documented_layout(store, bits, pixels):
    """qnn_pack_f32 against words built in numpy from the layout rules of include/qnn_abi.h (so pack is checked without
    unpack), pad fields asserted zero (the dense BIN kernel counts on it), and qnn_unpack_f32 fed numpy-built words."""
    for c in T.pack_cases():
        if (c["store"], c["bits"], c["pixels"]) != (store, bits, pixels):
            continue
        C = c["C"]
        codes = T.pack_codes(c)
        values = T.pack_values(c, codes)
        want = T.pack_words(codes, store)
        assert not (want == T.PACKED_FILL).any(), c["id"]
        xd = dev(values)
        got = _pack_into(xd, pixels, C, _abi.FN_GRID, bits, store, c["id"])
        assert not (got & T.pad_field_mask(store, C)).any(), c["id"] + ": pad fields are not zero"
        np.testing.assert_array_equal(got, want, err_msg=c["id"])
        out = Guarded(pixels, C, False)
        _abi.check(_abi.load().qnn_unpack_f32(_abi.ptr(dev_words(want)), out.ptr, pixels, C, store, bits, _abi.stream_ptr()),
                   "qnn_unpack_f32")
        out.check(c["id"] + " unpack")
        np.testing.assert_array_equal(host(out.region()), values, err_msg=c["id"] + " unpack")
        if pixels in (65, 4097) and store != T.STORE_T2:
            # the activation fused into the pack: pre-activations around the grid, the clip points and binary_tanh's threshold
            pre = T.act_values(pixels * C, bits, c["seed"]).reshape(pixels, C)
            if store == T.STORE_BIN:
                act, fn = O.binary_tanh(pre), _abi.FN_BINARY_TANH
                acodes = np.rint(act).astype(np.int64)
            else:
                act, fn = O.quantized_tanh(pre, bits), _abi.FN_QUANTIZED_TANH
                acodes = np.rint(act.astype(np.float64) * 2.0 ** (bits - 1)).astype(np.int64)
            got = _pack_into(dev(pre), pixels, C, fn, bits, store, c["id"] + " fused activation")
            np.testing.assert_array_equal(got, T.pack_words(acodes, store), err_msg=c["id"] + " fused activation")


# ---------------------------------------------------------------------------------------------------------------------
# elementwise activations
# ---------------------------------------------------------------------------------------------------------------------
def _act_call(fn, nb, xptr, yptr, n):
    lib = _abi.load()
    if fn == "binary_tanh":
        _abi.check(lib.qnn_binary_tanh_f32(xptr, yptr, n, _abi.stream_ptr()), "qnn_binary_tanh_f32")
    else:
        _abi.check(lib.qnn_quantized_tanh_f32(xptr, yptr, n, nb, _abi.stream_ptr()), "qnn_quantized_tanh_f32")


def _margin_tensor(values, off, fill_bits=NAN_FILL):
    """A fresh (256-byte aligned) int32 tensor [off fill elements | values | 4 fill elements] and the pointer to `values`."""
    n = values.size
    t = torch.full((off + n + 4,), fill_bits, dtype=torch.int32, device="cuda")
    t[off:off + n] = dev(values.view(np.int32))
    return t, ctypes.c_void_p(t.data_ptr() + 4 * off)


def _margins_untouched(t, off, n, fill_bits=NAN_FILL):
    return bool((t[:off] == fill_bits).all()) and bool((t[off + n:] == fill_bits).all())


@pytest.mark.parametrize("fn,nb", T.ACT_FNS, ids=["%s%d" % (f[0], b) for f, b in T.ACT_FNS])
def test_activations_at_every_length_and_pointer_offset(fn, nb):
    """binary_tanh / quantized_tanh at lengths around the float4 body and the block size (n % 4 in {0, 1, 2, 3}; the length
    at which the strided loop would wrap is stated in tail_cases.py), on views at element offsets 0..3 of a larger tensor
    (4-byte-aligned pointers into the float4 path) with the elements on both sides checked untouched, and in place."""
    for n in T.ACT_LENGTHS:
        x = T.act_values(n, nb, 11 * n + nb)
        want = T.act_reference(fn, nb, x)
        for xoff in T.ACT_OFFSETS:
            for yoff in T.ACT_OFFSETS:
                xt, xp = _margin_tensor(x, xoff)
                yt, yp = _margin_tensor(np.full(n, np.uint32(NAN_FILL)).view(F32), yoff)
                _act_call(fn, nb, xp, yp, n)
                torch.cuda.synchronize()
                what = "%s nb=%d n=%d x offset %d y offset %d" % (fn, nb, n, xoff, yoff)
                assert _margins_untouched(yt, yoff, n), "elements next to the output view were written: " + what
                got = host(yt[yoff:yoff + n]).view(F32)
                np.testing.assert_array_equal(got, want, err_msg=what)
                assert torch.equal(xt[xoff:xoff + n], dev(x.view(np.int32))) and _margins_untouched(xt, xoff, n), what
            xt, xp = _margin_tensor(x, xoff)                                   # in place
            _act_call(fn, nb, xp, xp, n)
            torch.cuda.synchronize()
            what = "%s nb=%d n=%d in place at offset %d" % (fn, nb, n, xoff)
            assert _margins_untouched(xt, xoff, n), what
            np.testing.assert_array_equal(host(xt[xoff:xoff + n]).view(F32), want, err_msg=what)


def _ternary(x, ws, yoff=0):
    n = x.size
    xd = dev(x)
    yt, yp = _margin_tensor(np.full(n, np.uint32(NAN_FILL)).view(F32), yoff)
    _abi.check(_abi.load().qnn_ternary_tanh_f32(_abi.ptr(xd), yp, n, _abi.ptr(ws), _abi.stream_ptr()), "qnn_ternary_tanh_f32")
    torch.cuda.synchronize()
    assert _margins_untouched(yt, yoff, n), "ternary_tanh wrote next to its output (n = %d)" % n
    return host(yt[yoff:yoff + n]).view(F32)


def test_ternary_tanh_lengths_thresholds_and_workspace_reuse():
    """ternary_tanh bit-exact against the oracle at lengths around a wave, on all zeros, and on a tensor with a known share
    of elements exactly AT the cutoff (+t -> 0, -t -> -1); the 16-byte workspace starts out as garbage and is re-used from
    call to call without clearing: qnn_ternary_abs_sum_f32 resets it."""
    ws = torch.full((4,), T.PACKED_FILL, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(8)
    for n in T.TERNARY_LENGTHS:
        x = rng.standard_normal(n).astype(F32)
        np.testing.assert_array_equal(_ternary(x, ws, yoff=n % 4), O.ternary_tanh(x), err_msg="n = %d" % n)
    z = np.zeros(1000, dtype=F32)
    np.testing.assert_array_equal(_ternary(z, ws), O.ternary_tanh(z))
    for n in (64, 66, 4096, 10 ** 6):
        x, t = T.ternary_threshold_tensor(n, n)
        got = _ternary(x, ws)
        np.testing.assert_array_equal(got, O.ternary_tanh(x), err_msg="threshold tensor, n = %d" % n)
        assert (got[x == t] == 0).all() and (got[x == -t] == -1).all() and (x == t).sum() == 16 and (x == -t).sum() == 16
    # the two halves with an explicit re-use: the second sum must not include the first
    lib = _abi.load()
    a, b = dev(rng.standard_normal(5000).astype(F32)), dev(rng.standard_normal(777).astype(F32))
    for t_ in (a, b):
        _abi.check(lib.qnn_ternary_abs_sum_f32(_abi.ptr(t_), t_.numel(), _abi.ptr(ws), _abi.stream_ptr()), "abs_sum")
        got = host(ws).view(np.float64)
        want = np.abs(np.clip(host(t_), -1, 1)).astype(np.float64).sum()
        assert got[1] == t_.numel() and abs(got[0] - want) <= 1e-12 * want, (got, want)
