"""The depthwise convolution on the GPU (include/qnn_abi_depthwise.h, csrc/qnn_depthwise.hip) against the numpy reference
of depthwise_cases.py, bit for bit, with the kernel name asserted: every store, channel count, window, stride, padding,
dilation and depth multiplier of the case table with the input's spare bits set, both pointers moved off their 16-byte
alignment, every weight kind, every epilogue, both sides of the 16-bit bound, both forms beyond one workgroup and the
16-bit-lane form beyond two row blocks (D.multitask_cases()), the block-diagonal expansion through
qnn_conv2d_forward, every refusal, the empty batch, and the layer classes."""
import ctypes

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi

import depthwise_cases as D

pytestmark = pytest.mark.gpu
ENTRIES = _abi.EXPORTS_DEPTHWISE          # read at import: without the entries nothing below means anything
FILL = 0x5A5A5A5A
NAMES = {D.F32: "f32", D.BIN: "bin", D.T2: "t2", D.I4: "i4", D.I8: "i8"}


def dev(a, misalign=False):
    a = np.array(a, order="C")
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    if not misalign:
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.full((t.numel() + 4,), FILL, dtype=torch.int32, device="cuda").view(t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def host(t):
    torch.cuda.synchronize()
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def handle(c, kernel, bias, store=None):
    return _abi.DepthwiseWeights(c["wkind"], c["wbits"], 1.0, dev(kernel), dev(bias) if bias is not None else None,
                                 c["stride"], c["same"], c["store"] if store is None else store, dilation=c["dil"])


def expected_name(c, w):
    if c["store"] in (D.I4, D.I8):
        return "depthwise_%s%s" % (NAMES[c["store"]], "" if D.takes_pk16(c) else "_plain")
    return "depthwise_" + NAMES[c["store"]]


def run_case(c, inputs=None, seed=0):
    x, kernel, bias, bn = inputs if inputs is not None else D.make_inputs(c, seed)
    N, H, W = c["map"]
    cout = c["C"] * c["M"]
    want = D.reference(c, x, kernel, bias, bn)
    w = handle(c, kernel, bias)
    np.testing.assert_array_equal(host(w.dequant()).view(np.uint32),
                                  D.quantize_weights(kernel, c["wkind"], c["wbits"])[0].view(np.uint32))
    if c["store"] == D.F32:
        xd = dev(x, c["misalign"])
    else:
        xd = dev(D.encode(x, c["store"], spare=np.random.RandomState(7)).reshape(N * H * W, -1), c["misalign"])
    Ho, Wo = want.shape[1:3]
    assert (Ho, Wo) == w.out_hw(H, W)
    if c["out_store"] == D.F32:
        shape, dt = (N, Ho, Wo, cout), np.float32
    else:
        shape, dt = (N * Ho * Wo, D.words(c["out_store"], cout)), np.uint32
    out = dev(np.full(shape, FILL, np.uint32).view(dt), c["misalign"])
    bnd = (dev(bn[0]), dev(bn[1])) if bn is not None else (None, None)
    y, ho, wo = _abi.depthwise(w, xd, c["store"], c["x_bits"], N, H, W, bnd[0], bnd[1], c["fn"], c["act_bits"],
                               c["out_store"], out=out)
    assert _abi.last_kernel() == expected_name(c, w)
    assert (ho, wo) == (Ho, Wo)
    got = host(y)
    if c["out_store"] == D.F32:
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    else:
        codes, spare = D.decode(got.reshape(N, Ho, Wo, -1), c["out_store"], cout)
        np.testing.assert_array_equal(codes, want)
        assert not spare.any(), "spare bits of the last word are not zero"
    return got


@pytest.mark.parametrize("c", D.geometry_cases(), ids=D.case_id)
def test_geometry(c):
    run_case(c)


@pytest.mark.parametrize("c", D.weight_cases(), ids=D.case_id)
def test_weight_kinds(c):
    run_case(c)


EPILOGUE_IDS = [D.case_id(c) for c in D.epilogue_cases()]
EPILOGUE_STORES = [c["store"] for c in D.epilogue_cases()]


@pytest.mark.parametrize("c", D.epilogue_cases(), ids=D.case_id)
def test_epilogues(c):
    import test_gpu_sideconv_grid as grid
    try:
        run_case(c)
    finally:
        # on exact ties, zeros and clip edges: the groups of sideconv_grid_cases.py that this id carries (its own input store)
        grid.run_hosted("dw", EPILOGUE_STORES, EPILOGUE_IDS.index(D.case_id(c)))


@pytest.mark.parametrize("c", D.bound_cases(), ids=D.case_id)
def test_both_sides_of_the_16_bit_bound(c):
    # extreme codes everywhere: the largest sums the widths allow
    x, kernel, bias, bn = D.make_inputs(c)
    x = np.where(np.random.RandomState(3).rand(*x.shape) < 0.7, -(1 << (c["x_bits"] - 1)), x)
    kernel = np.where(np.random.RandomState(4).rand(*kernel.shape) < 0.7, np.float32(-1), kernel).astype(np.float32)
    run_case(c, (x, kernel, bias, bn))
    _beyond_two_row_blocks_and_one_workgroup(c)


def test_constructed_overflow_takes_the_32_bit_form():
    c, x, kernel = D.overflow_case()
    got = run_case(c, (x, kernel, None, None))
    assert _abi.last_kernel() == "depthwise_i8_plain"
    assert got.max() == np.float32(9.0)          # 147456 * 2^-14


def test_aligned_and_misaligned_agree():
    for store, chans in D.CHANNELS.items():
        c = D._case(store, max(chans))
        a = run_case(c)
        b = run_case(dict(c, misalign=True))
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    # the same on more than 256 items (the plain case of D.multitask_cases()): blockIdx.x > 0 in the item decode
    cases = [c for c in D.multitask_cases() if not D.takes_pk16(c)]
    assert [c["misalign"] for c in cases] == [False, True]
    a, b = (run_multitask(c) for c in cases)
    assert _abi.last_kernel() == "depthwise_bin"
    np.testing.assert_array_equal(a, b)


def run_multitask(c):
    """run_case on a case of D.multitask_cases() with its own seed; on top of it, no word of the output is the pattern
    laid under it (test_depthwise_cpu.py: no expected word is).  Returns the codes."""
    try:
        got = run_case(c, D.make_inputs(c, c["seed"]))
        assert not (got == FILL).any(), "an output word was not written"
    except AssertionError as e:
        raise AssertionError("case %s: %s" % (D.case_id(c), e)) from e
    return D.decode(got, c["out_store"], c["C"])[0]          # (pixels, words) -> (pixels, C)


def _beyond_two_row_blocks_and_one_workgroup(host):
    """Behind the first 16-bit-lane case of D.bound_cases() on each store, the cases of D.multitask_cases() on that store:
    blockIdx.x > 0, three and four row blocks per image with a last block of 2, 4 and 1 rows, n > 0 behind them -- against
    the reference and, the same 4-bit codes written to the other packed store, the plain form.  Every case runs; the
    failures are reported together, each under its case id."""
    store = host["store"]
    first = next(c for c in D.bound_cases() if c["store"] == store and D.takes_pk16(c))
    if D.case_id(host) != D.case_id(first):
        return
    cases = [c for c in D.multitask_cases() if c["store"] == store and D.takes_pk16(c)]
    assert len(cases) == (4 if store == D.I4 else 3)
    failures = []
    for c in cases:
        try:
            fast = run_multitask(c)
            assert _abi.last_kernel() == "depthwise_" + NAMES[store], D.case_id(c)
            plain = run_multitask(dict(c, out_store=D.I8 if store == D.I4 else D.I4))
            assert _abi.last_kernel() == "depthwise_%s_plain" % NAMES[store], D.case_id(c)
            np.testing.assert_array_equal(fast, plain, err_msg=D.case_id(c))
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "%d of %d multitask cases:\n%s" % (len(failures), len(cases), "\n".join(failures))


@pytest.mark.parametrize("store,C,wbits,x_bits,M", [(D.I4, 9, 4, 4, 1), (D.I4, 32, 2, 4, 1), (D.I8, 5, 8, 8, 1),
                                                    (D.I8, 16, 4, 8, 1), (D.I4, 8, 4, 4, 2)])
@pytest.mark.parametrize("stride,same", [(1, True), (2, False)])
def test_equals_the_block_diagonal_full_convolution(store, C, wbits, x_bits, M, stride, same):
    """Quantized weights only: quantize(0) = 0, so the expansion is exact.  ternarize is NOT elementwise -- its cutoff is
    0.7 * mean|W| over the whole kernel (ternary_ops.py:15-30) and the zeros of the expansion move it -- and binarize(0)
    is +-1, so those two kinds have no expanded form; a float32 input would sum the zero products in another order."""
    c = D._case(store, C, M=M, wbits=wbits, x_bits=x_bits, stride=stride, same=same)
    x, kernel, bias, bn = D.make_inputs(c)
    N, H, W = c["map"]
    xd = dev(D.encode(x, store).reshape(N * H * W, -1))
    bnd = (dev(bn[0]), dev(bn[1]))
    y, Ho, Wo = _abi.depthwise(handle(c, kernel, bias), xd, store, x_bits, N, H, W, bnd[0], bnd[1], c["fn"], c["act_bits"], store)
    full = _abi.Weights(D.W_QUANT, wbits, 1.0, dev(D.expand_block_diagonal(kernel)), dev(bias), stride, same, store)
    z, Hz, Wz = _abi.conv2d(full, xd, store, x_bits, N, H, W, bnd[0], bnd[1], c["fn"], c["act_bits"], 1, store)
    assert (Ho, Wo) == (Hz, Wz)
    np.testing.assert_array_equal(host(y), host(z))


def _epi(**kw):
    e = _abi.make_epilogue(None, None, _abi.FN_NONE, 0, 1, _abi.STORE_F32, flags=0)
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _forward_rc(w, x, x_store, x_bits, N, H, W, epi, y):
    lib = _abi.load()
    rc = lib.qnn_depthwise_forward(w.handle if w is not None else None, _abi.ptr(x), x_store, x_bits, N, H, W,
                                   ctypes.byref(epi), _abi.ptr(y), _abi.stream_ptr())
    return rc, lib.qnn_last_error().decode()


def test_refusals_and_empty_batch():
    EINVAL, EUNSUP = -1, -2
    c = D._case(D.I4, 8)
    x, kernel, bias, bn = D.make_inputs(c)
    N, H, W = c["map"]
    w = handle(c, kernel, bias)
    xd = dev(D.encode(x, D.I4).reshape(N * H * W, -1))
    y = torch.zeros((N, H, W, 8), dtype=torch.float32, device="cuda")
    some = torch.zeros(64, dtype=torch.float32, device="cuda")
    ok = (w, xd, D.I4, 4, N, H, W)
    assert _forward_rc(*ok, _epi(), y)[0] == 0
    for field, value in (("pool", 2), ("res", some.data_ptr()), ("fold", some.data_ptr()), ("proj", some.data_ptr()),
                         ("trick_s", 2.0), ("flags", 1)):
        rc, msg = _forward_rc(*ok, _epi(**{field: value}), y)
        assert rc == EUNSUP and field in msg, (field, rc, msg)
    for xs in (_abi.STORE_U8, _abi.STORE_F32_IMAGE, _abi.STORE_F32_UNIT):
        rc, msg = _forward_rc(w, xd, xs, 4, N, H, W, _epi(), y)
        assert rc == EUNSUP and "x_store" in msg
    for fn in _abi.MAXACT_FNS:
        assert _forward_rc(*ok, _epi(fn=fn, act_bits=4), y)[0] == EUNSUP
    # QNN_EINVAL
    assert _forward_rc(w, None, D.I4, 4, N, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, D.I4, 4, N, H, W, _epi(), None)[0] == EINVAL
    assert _forward_rc(None, xd, D.I4, 4, N, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, D.I4, 4, -1, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, D.I4, 4, N, 0, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, D.I8, 4, N, H, W, _epi(), y)[0] == EINVAL          # not the handle's store
    assert _forward_rc(w, xd, D.I4, 5, N, H, W, _epi(), y)[0] == EINVAL          # x_bits beyond the store
    assert _forward_rc(w, xd, D.I4, 0, N, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, 3, 4, N, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(fn=_abi.FN_TERNARY_TANH), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(fn=_abi.FN_LEAKY_RELU, out_store=D.I4), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(fn=_abi.FN_QUANTIZED_TANH, act_bits=8, out_store=D.I4), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(fn=_abi.FN_QUANTIZED_TANH, act_bits=4, out_store=D.BIN), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(out_store=D.T2), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(bn_inv=some.data_ptr()), y)[0] == EINVAL
    assert _forward_rc(w, xd, D.I4, 4, N, H, W, _epi(), xd)[0] == EINVAL          # y overlaps x
    valid5 = handle(dict(c, window=(5, 5), same=False), np.zeros((5, 5, 8, 1), np.float32), None)
    assert _forward_rc(valid5, xd, D.I4, 4, N, 4, 4, _epi(), y)[0] == EINVAL     # empty output
    # 2^31 output words: refused before any pointer is used
    rc, msg = _forward_rc(w, xd, D.I4, 4, 1 << 20, 64, 64, _epi(), y)
    assert rc == EUNSUP and "2^31" in msg
    # N == 0: QNN_OK without a launch, null pointers allowed
    assert _forward_rc(w, None, D.I4, 4, 0, H, W, _epi(), None)[0] == 0
    # prepack
    k = dev(kernel)
    lib = _abi.load()

    def prepack(wkind=D.W_QUANT, wbits=4, kh=3, kw=3, C=8, M=1, stride=1, dh=1, dw=1, store=D.I4, kern=k):
        h = ctypes.c_void_p(None)
        rc = lib.qnn_depthwise_prepack(wkind, wbits, 1.0, _abi.ptr(kern), kh, kw, C, M, None, stride, 1, dh, dw, store,
                                       _abi.stream_ptr(), ctypes.byref(h))
        if rc == 0:
            lib.qnn_depthwise_free(h)
        return rc
    assert prepack() == 0
    assert prepack(kh=8) == EUNSUP and prepack(kw=8) == EUNSUP
    assert prepack(stride=3) == EUNSUP and prepack(stride=0) == EINVAL
    assert prepack(dh=2, stride=2) == EUNSUP and prepack(dw=65) == EUNSUP and prepack(dh=0) == EINVAL
    assert prepack(C=0) == EINVAL and prepack(M=0) == EINVAL and prepack(kern=None) == EINVAL
    assert prepack(wbits=8) == EINVAL and prepack(store=D.BIN) == EINVAL and prepack(wkind=D.W_FLOAT) == EINVAL
    assert prepack(wkind=7) == EINVAL and prepack(store=3) == EINVAL


LAYER_CASES = [
    (qnn_amd.DepthwiseConv2D, {}, None, D.W_FLOAT, 0),
    (qnn_amd.DepthwiseConv2D, {"depth_multiplier": 2, "strides": 2, "padding": "same", "use_bias": False}, None, D.W_FLOAT, 0),
    (qnn_amd.BinaryDepthwiseConv2D, {"padding": "same"}, "binary", D.W_BINARY, 1),
    (qnn_amd.QuantizedDepthwiseConv2D, {"nb": 4, "padding": "same"}, ("quantized", 4), D.W_QUANT, 4),
    (qnn_amd.QuantizedDepthwiseConv2D, {"nb": 4, "dilation_rate": (1, 2)}, None, D.W_QUANT, 4),
    (qnn_amd.TernaryDepthwiseConv2D, {"padding": "same", "depth_multiplier": 3}, "ternary", D.W_TERNARY, 1),
]


@pytest.mark.parametrize("cls,kw,domain,wkind,wbits", LAYER_CASES)
def test_layer_classes(cls, kw, domain, wkind, wbits):
    rs = np.random.RandomState(5)
    N, H, W, C = 2, 5, 7, 9
    layer = cls((3, 3), input_domain=domain, **kw)
    layer.build((None, H, W, C))
    M = layer.depth_multiplier
    kernel = (rs.randint(-64, 65, (3, 3, C, M)) / 64.0).astype(np.float32)
    bias = (rs.randint(-8, 9, C * M) / 16.0).astype(np.float32)
    layer.set_weights([kernel, bias] if layer.use_bias else [kernel])
    got_w = layer.get_weights()
    np.testing.assert_array_equal(got_w[0], kernel)
    if domain == "binary":
        x = rs.choice([-1.0, 1.0], (N, H, W, C)).astype(np.float32)
    elif domain == "ternary":
        x = rs.randint(-1, 2, (N, H, W, C)).astype(np.float32)
    elif domain is not None:
        x = (rs.randint(-8, 8, (N, H, W, C)) / 8.0).astype(np.float32)
    else:
        x = (rs.randint(-64, 65, (N, H, W, C)) / 32.0).astype(np.float32)
    q = D.quantize_weights(kernel, wkind, wbits)[0]
    np.testing.assert_array_equal(host(layer.quantized_kernel()), q)
    # grid inputs and dyadic weights: the float64 sum of the reference is exact, whichever path the layer took
    v = D.dw_sum(x, q, layer.strides[0], layer.padding == "same", layer.dilation_rate, np.float64).astype(np.float32)
    want = D.chain(v, bias if layer.use_bias else None, None, D.FN_NONE, 0, D.F32)
    y = host(layer(torch.from_numpy(x).cuda()))
    assert y.shape == layer.compute_output_shape((N, H, W, C))
    np.testing.assert_array_equal(y.view(np.uint32), want.view(np.uint32))


# ---- capture, the spec op on the engines ----------------------------------------------------------------------------------
def test_forward_call_is_capturable():
    """No allocation, host read or synchronisation in qnn_depthwise_forward: it is captured into a hipGraph and replayed on
    new input in the same buffers."""
    c = D._case(D.I4, 32)
    x, kernel, bias, bn = D.make_inputs(c)
    N, H, W = c["map"]
    w = handle(c, kernel, bias)
    bnd = (dev(bn[0]), dev(bn[1]))
    xd = dev(D.encode(x, D.I4).reshape(N * H * W, -1))
    out = torch.zeros((N * H * W, D.words(D.I4, 32)), dtype=torch.int32, device="cuda")
    epi = _abi.make_epilogue(bnd[0], bnd[1], c["fn"], c["act_bits"], 1, D.I4, flags=0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _abi.depthwise(w, xd, D.I4, 4, N, H, W, out_store=D.I4, out=out, epilogue=epi)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _abi.depthwise(w, xd, D.I4, 4, N, H, W, out_store=D.I4, out=out, epilogue=epi)
    x2 = D.make_inputs(c, seed=1)[0]
    xd.copy_(dev(D.encode(x2, D.I4).reshape(N * H * W, -1)))
    out.zero_()
    graph.replay()
    codes, _ = D.decode(host(out).reshape(N, H, W, -1), D.I4, 32)
    np.testing.assert_array_equal(codes, D.reference(c, x2, kernel, bias, bn))


def separable_spec(kind="quantized", C=8, F=16, M=1, seed=0):
    rs = np.random.RandomState(40 + seed)
    dyad = lambda n: (2.0 ** rs.randint(-2, 2, n)).astype(np.float32)           # noqa: E731

    def bn(n):
        return {"op": "bn", "eps": 0.0, "gamma": dyad(n), "beta": (rs.randint(-8, 9, n) / 32.0).astype(np.float32),
                "mean": np.zeros(n, np.float32), "var": np.ones(n, np.float32)}
    dw = {"op": "dwconv", "kind": kind, "kernel": (rs.randint(-64, 65, (3, 3, C, M)) / 64.0).astype(np.float32),
          "bias": (rs.randint(-8, 9, C * M) / 16.0).astype(np.float32), "strides": (1, 1), "padding": "same",
          "dilation": (1, 1), "depth_multiplier": M, "nb": 4, "H": 1.0}
    pw = {"op": "conv", "kind": "quantized", "nb": 4, "kernel": (rs.randint(-64, 65, (1, 1, C * M, F)) / 64.0).astype(np.float32),
          "bias": (rs.randint(-8, 9, F) / 16.0).astype(np.float32), "strides": (1, 1), "padding": "same"}
    return [{"op": "act", "fn": "quantized_tanh", "nb": 4}, dw, bn(C * M), {"op": "act", "fn": "quantized_tanh", "nb": 4},
            pw, bn(F)]


def separable_reference(spec, x):
    act, dw, bn1, _, pw, bn2 = spec
    wk = {"quantized": D.W_QUANT, "binary": D.W_BINARY, "ternary": D.W_TERNARY}[dw["kind"]]
    c = dict(store=D.I4, stride=1, same=True, dil=(1, 1), wkind=wk, wbits=4, x_bits=4, fn=D.FN_QUANTIZED_TANH, act_bits=4,
             out_store=D.I4)
    codes = D.qact_code(D.FN_QUANTIZED_TANH, x, 8).astype(np.int64)
    mid = D.reference(c, codes, dw["kernel"], dw["bias"], (bn1["gamma"], bn1["beta"]))
    wq = D.quantize_weights(pw["kernel"], D.W_QUANT, 4)[1][0, 0]
    v = ((mid @ wq).astype(np.float32) * np.float32(2.0 ** -6)).astype(np.float32)
    return D.chain(v, pw["bias"], (bn2["gamma"], bn2["beta"]), D.FN_NONE, 0, D.F32)


def _inputs(seed=0, C=8):
    rs = np.random.RandomState(60 + seed)
    return (rs.randint(-40, 41, (2, 5, 7, C)) / 32.0).astype(np.float32)


@pytest.mark.parametrize("kind,M", [("quantized", 1), ("quantized", 2), ("binary", 1), ("ternary", 1)])
def test_separable_block_on_the_engines(kind, M, monkeypatch):
    from qnn_amd import engine, nets
    spec = separable_spec(kind, M=M)
    x = _inputs()
    want = separable_reference(spec, x)
    calls = []
    for fname in ("pack", "unpack", "depthwise", "conv2d", "conv2d_f32in"):
        real = getattr(_abi, fname)

        def wrapped(*a, _real=real, _name=fname, **kw):
            r = _real(*a, **kw)
            calls.append((_name, _abi.last_kernel() if _name in ("depthwise", "conv2d", "conv2d_f32in") else None,
                          a[2] if _name in ("depthwise", "conv2d") else None))
            return r
        monkeypatch.setattr(_abi, fname, wrapped)
    gm = engine.GraphModel(spec)
    gm.kernel_log = []
    y = host(gm(torch.from_numpy(x).cuda()))
    np.testing.assert_array_equal(y.view(np.uint32), want.view(np.uint32))
    # codes stay packed from the producer's pack, through dwconv, into the 1x1 conv: one pack, no unpack, both contractions
    # read int4 words, and the depthwise kernel is the packed one
    assert [c[0] for c in calls] == ["pack", "depthwise", "conv2d"], calls
    assert calls[1][1] == ("depthwise_i4" if M == 1 else "depthwise_i4_plain") and calls[1][2] == D.I4
    assert calls[2][2] == D.I4 and "f32in" not in calls[2][1]
    assert gm.kernel_log == ["pack", calls[1][1]]
    monkeypatch.undo()
    lm = engine.LayerModel(spec)
    np.testing.assert_array_equal(host(lm(torch.from_numpy(x).cuda())).view(np.uint32), want.view(np.uint32))
    assert isinstance(nets.Model(None, spec).engine, engine.GraphModel)
    for cls in (engine.FusedModel, engine.ResidualFusedModel):
        with pytest.raises(_abi.NotFusable, match="dwconv"):
            cls(spec)


def test_graphmodel_capture_and_replay():
    from qnn_amd import engine
    spec = separable_spec()
    gm = engine.GraphModel(spec)
    xs = torch.from_numpy(_inputs(0)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gm(xs)                                       # prepacks the weights outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = gm(xs)
    x2 = _inputs(1)
    xs.copy_(torch.from_numpy(x2).cuda())
    graph.replay()
    np.testing.assert_array_equal(host(ys).view(np.uint32), separable_reference(spec, x2).view(np.uint32))


def test_float_dwconv_and_scaled_codes():
    """A float dwconv (what the importer emits) on both engines, and behind a batch-scaled activation: with
    scaled_codes=True the dwconv still reads the float32 tensor."""
    from qnn_amd import engine
    rs = np.random.RandomState(70)
    k = (rs.randint(-64, 65, (3, 3, 5, 2)) / 64.0).astype(np.float32)
    b = (rs.randint(-8, 9, 10) / 16.0).astype(np.float32)
    dw = {"op": "dwconv", "kind": "float", "kernel": k, "bias": b, "strides": (2, 2), "padding": "same", "dilation": (1, 1),
          "depth_multiplier": 2, "H": 1.0}
    x = _inputs(2, C=5)
    c = dict(store=D.F32, stride=2, same=True, dil=(1, 1), wkind=D.W_FLOAT, fn=D.FN_NONE, out_store=D.F32)
    want = D.reference(c, x, k, b, None)
    for cls in (engine.GraphModel, engine.LayerModel):
        np.testing.assert_array_equal(host(cls([dw])(torch.from_numpy(x).cuda())).view(np.uint32), want.view(np.uint32))
    spec = [{"op": "act", "fn": "quantized_maxrelu", "nb": 4}, dict(dw, kind="quantized", nb=4)]
    xd = torch.from_numpy(x).cuda()
    plain, scaled = engine.GraphModel(spec), engine.GraphModel(spec, scaled_codes=True)
    scaled.kernel_log = []
    np.testing.assert_array_equal(host(plain(xd)), host(scaled(xd)))
    assert scaled.kernel_log == ["depthwise_f32"]
