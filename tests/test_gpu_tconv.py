"""The transposed convolution on the GPU (include/qnn_abi_tconv.h, csrc/qnn_tconv.hip) against the numpy reference of
tconv_cases.py, bit for bit, with the kernel name asserted wherever a route is claimed: the plain form on every store,
window, stride, padding, map and channel count of the case table with the input's spare bits set, pointers moved off
their 16-byte alignment, every weight kind and epilogue; the matrix-pipe form against the reference and against the plain
form, on one and on several wave tasks per phase; the plain form beyond one workgroup; the route's edges;
every refusal; capture into a hipGraph; the layer classes; the spec op on the engines."""
import ctypes

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi

import tconv_cases as T

pytestmark = pytest.mark.gpu
ENTRIES = _abi.EXPORTS_TCONV              # read at import: without the entries nothing below means anything
FILL = 0x5A5A5A5A
NAMES = {T.F32: "f32", T.BIN: "bin", T.T2: "t2", T.I4: "i4", T.I8: "i8"}


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
    return _abi.TConvWeights(c["wkind"], c["wbits"], 1.0, dev(kernel), dev(bias) if bias is not None else None,
                             c["stride"], c["same"], c["store"] if store is None else store)


def expected_name(c):
    if c["store"] in (T.I4, T.I8):
        return "tconv_%s_%s" % (NAMES[c["store"]], "mfma" if T.takes_mfma(c) else "plain")
    return "tconv_" + NAMES[c["store"]]


def run_case(c, inputs=None, seed=0, w=None, check_weights=True):
    """One forward call of case `c` compared with the reference; returns the decoded output (values or codes)."""
    x, kernel, bias, bn = inputs if inputs is not None else T.make_inputs(c, seed)
    N, H, W = c["map"]
    cout = c["Cout"]
    want = T.reference(c, x, kernel, bias, bn)
    w = handle(c, kernel, bias) if w is None else w
    if check_weights:
        np.testing.assert_array_equal(host(w.dequant()).view(np.uint32),
                                      T.quantize_weights(kernel, c["wkind"], c["wbits"])[0].view(np.uint32))
    if c["store"] == T.F32:
        xd = dev(x, c["misalign"])
    else:
        xd = dev(T.encode(x, c["store"], spare=np.random.RandomState(7)).reshape(N * H * W, -1), c["misalign"])
    Ho, Wo = want.shape[1:3]
    assert (Ho, Wo) == w.out_hw(H, W)
    if c["out_store"] == T.F32:
        shape, dt = (N, Ho, Wo, cout), np.float32
    else:
        shape, dt = (N * Ho * Wo, T.words(c["out_store"], cout)), np.uint32
    out = dev(np.full(shape, FILL, np.uint32).view(dt), c["misalign"])
    bnd = (dev(bn[0]), dev(bn[1])) if bn is not None else (None, None)
    y, ho, wo = _abi.tconv(w, xd, c["store"], c["x_bits"], N, H, W, bnd[0], bnd[1], c["fn"], c["act_bits"], c["out_store"],
                           out=out)
    assert _abi.last_kernel() == expected_name(c)
    assert (ho, wo) == (Ho, Wo)
    got = host(y)
    if c["out_store"] == T.F32:
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        return got
    codes, spare = T.decode(got.reshape(N, Ho, Wo, -1), c["out_store"], cout)
    np.testing.assert_array_equal(codes, want)
    assert not spare.any(), "spare bits of the last word are not zero"
    return codes


# ---- the plain form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.geometry_cases(), ids=T.case_id)
def test_geometry(c):
    run_case(c)


@pytest.mark.parametrize("c", T.channel_cases(), ids=T.case_id)
def test_channel_counts(c):
    run_case(c)


@pytest.mark.parametrize("c", T.weight_cases(), ids=T.case_id)
def test_weight_kinds(c):
    run_case(c)


EPILOGUE_IDS = [T.case_id(c) for c in T.epilogue_cases()]
EPILOGUE_STORES = [c["store"] for c in T.epilogue_cases()]


@pytest.mark.parametrize("c", T.epilogue_cases(), ids=T.case_id)
def test_epilogues(c):
    import test_gpu_sideconv_grid as grid
    try:
        run_case(c)
    finally:
        # on exact ties, zeros and clip edges: the groups of sideconv_grid_cases.py that this id carries (its own input store)
        grid.run_hosted("tc", EPILOGUE_STORES, EPILOGUE_IDS.index(T.case_id(c)))


def test_aligned_and_misaligned_agree():
    """4-byte-aligned pointers take V = 1, 16-byte-aligned ones V = 4 where the words per pixel divide by 4."""
    for c in (T._case(T.F32, 3, 8), T._case(T.BIN, 33, 128), T._case(T.T2, 33, 32), T._case(T.I4, 9, 32), T._case(T.I8, 9, 16),
              T._case(T.I4, 9, 17)):
        a = run_case(c)
        b = run_case(dict(c, misalign=True))
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                      b.view(np.uint32) if b.dtype == np.float32 else b)
    # the same on more than 256 items (the plain case of T.multitask_cases()): blockIdx.x > 0 in the item decode
    cases = [c for c in T.multitask_cases() if not T.takes_mfma(c)]
    assert [c["misalign"] for c in cases] == [False, True]
    a, b = (run_multitask(c) for c in cases)
    assert _abi.last_kernel() == "tconv_i8_plain"
    np.testing.assert_array_equal(a, b)


# ---- the matrix-pipe form ----------------------------------------------------------------------------------------------------
def _other_store(c):
    """The same call with the codes written to the OTHER packed store (act_bits fits both): out_store != x_store takes the
    plain form, the codes are the same."""
    other = T.I8 if c["store"] == T.I4 else T.I4
    return dict(c, out_store=other, act_bits=min(c["act_bits"], 4))


@pytest.mark.parametrize("c", T.mfma_cases(), ids=T.case_id)
def test_matrix_pipe_equals_reference_and_plain_form(c):
    c = dict(c, act_bits=4)                  # a width both stores hold, so the plain form can be forced by the store
    inputs = T.make_inputs(c)
    w = handle(c, inputs[1], inputs[2])
    fast = run_case(c, inputs, w=w)
    assert _abi.last_kernel() == "tconv_%s_mfma" % NAMES[c["store"]]
    plain = run_case(_other_store(c), inputs, w=w, check_weights=False)
    assert _abi.last_kernel() == "tconv_%s_plain" % NAMES[c["store"]]
    np.testing.assert_array_equal(fast, plain)
    # the same pointers moved off their alignment: the plain form again, at out_store == x_store
    off = run_case(dict(c, misalign=True), inputs, w=w, check_weights=False)
    assert _abi.last_kernel() == "tconv_%s_plain" % NAMES[c["store"]]
    np.testing.assert_array_equal(fast, off)
    _several_wave_tasks_per_phase(c)


def run_multitask(c, **kw):
    """run_case on a case of T.multitask_cases() with its own seed; on top of it, no word of the output is the pattern
    laid under it (test_tconv_cpu.py: no expected word is)."""
    try:
        codes = run_case(c, T.make_inputs(c, c["seed"]), **kw)
        assert not (T.encode(codes, c["out_store"]) == FILL).any(), "an output word was not written"
    except AssertionError as e:
        raise AssertionError("case %s: %s" % (T.case_id(c), e)) from e
    return codes


def _shape_key(c):
    return c["store"], c["window"], c["same"], c["Cin"], c["Cout"]


def _multitask_hosts():
    """(shape, map) of the first case of T.mfma_cases() on a (store, window, padding, Cin, Cout) -> the matrix-pipe cases of
    T.multitask_cases() on the same: every one of them runs behind exactly one test id of the matrix-pipe form."""
    first, hosts = {}, {}
    for c in T.mfma_cases():
        first.setdefault(_shape_key(c), (_shape_key(c), c["map"]))
    for m in T.multitask_cases():
        if T.takes_mfma(m):
            hosts.setdefault(first[_shape_key(m)], []).append(m)
    assert sum(len(v) for v in hosts.values()) == 17
    return hosts


MULTITASK_HOSTS = _multitask_hosts()


def _several_wave_tasks_per_phase(host):
    """The cases of T.multitask_cases() on the host's (store, window, padding, Cin, Cout): GT = 2 and 3 with n > 0, phases
    that end before a later task's first group next to a phase that does not -- against the reference and against the plain
    form.  Every case runs; the failures are reported together, each under its case id."""
    cases = MULTITASK_HOSTS.get((_shape_key(host), host["map"]), [])
    failures = []
    for c in cases:
        try:
            w = handle(c, *T.make_inputs(c, c["seed"])[1:3])
            fast = run_multitask(c, w=w)
            assert _abi.last_kernel() == "tconv_%s_mfma" % NAMES[c["store"]], T.case_id(c)
            off = run_multitask(dict(c, misalign=True), w=w, check_weights=False)
            assert _abi.last_kernel() == "tconv_%s_plain" % NAMES[c["store"]], T.case_id(c)
            np.testing.assert_array_equal(fast, off, err_msg=T.case_id(c))
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "%d of %d multitask cases:\n%s" % (len(failures), len(cases), "\n".join(failures))


@pytest.mark.parametrize("store,fn,act_bits,x_bits,wkind,wbits", [
    (T.I4, T.FN_BINARY_TANH, 0, 4, T.W_QUANT, 4), (T.I4, T.FN_QUANTIZED_RELU, 4, 2, T.W_QUANT, 2),
    (T.I4, T.FN_QUANTIZED_LEAKYRELU, 3, 4, T.W_TERNARY, 1), (T.I8, T.FN_QUANTIZED_TANH, 8, 8, T.W_QUANT, 8),
    (T.I8, T.FN_QUANTIZED_RELU, 6, 4, T.W_BINARY, 1), (T.I8, T.FN_BINARY_TANH, 0, 8, T.W_QUANT, 4)])
@pytest.mark.parametrize("bias,bn", [(True, True), (False, False)])
def test_matrix_pipe_epilogues_and_widths(store, fn, act_bits, x_bits, wkind, wbits, bias, bn):
    c = T._case(store, 64, 48, window=(4, 4), stride=2, same=True, map=(3, 2, 15), fn=fn, act_bits=act_bits, x_bits=x_bits,
                wkind=wkind, wbits=wbits, bias=bias, bn=bn)
    run_case(c)
    assert _abi.last_kernel() == "tconv_%s_mfma" % NAMES[store]


@pytest.mark.parametrize("c", T.boundary_cases(), ids=T.case_id)
def test_route_boundaries_take_the_plain_form(c):
    run_case(c)
    assert _abi.last_kernel() == "tconv_%s_plain" % NAMES[c["store"]]


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _epi(**kw):
    e = _abi.make_epilogue(None, None, _abi.FN_NONE, 0, 1, _abi.STORE_F32, flags=0)
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _forward_rc(w, x, x_store, x_bits, N, H, W, epi, y):
    lib = _abi.load()
    rc = lib.qnn_tconv_forward(w.handle if w is not None else None, _abi.ptr(x), x_store, x_bits, N, H, W,
                               ctypes.byref(epi), _abi.ptr(y), _abi.stream_ptr())
    return rc, lib.qnn_last_error().decode()


def test_refusals_and_empty_batch():
    EINVAL, EUNSUP = -1, -2
    c = T._case(T.I4, 8, 8)
    x, kernel, bias, bn = T.make_inputs(c)
    N, H, W = c["map"]
    w = handle(c, kernel, bias)
    xd = dev(T.encode(x, T.I4).reshape(N * H * W, -1))
    y = torch.zeros((N, 2 * H, 2 * W, 8), dtype=torch.float32, device="cuda")
    some = torch.zeros(64, dtype=torch.float32, device="cuda")
    ok = (w, xd, T.I4, 4, N, H, W)
    assert _forward_rc(*ok, _epi(), y)[0] == 0
    name = _abi.last_kernel()
    assert name == "tconv_i4_plain"
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
    assert _forward_rc(w, None, T.I4, 4, N, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, T.I4, 4, N, H, W, _epi(), None)[0] == EINVAL
    assert _forward_rc(None, xd, T.I4, 4, N, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, T.I4, 4, -1, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, T.I4, 4, N, 0, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, T.I8, 4, N, H, W, _epi(), y)[0] == EINVAL          # not the handle's store
    assert _forward_rc(w, xd, T.I4, 5, N, H, W, _epi(), y)[0] == EINVAL          # x_bits beyond the store
    assert _forward_rc(w, xd, T.I4, 0, N, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, 3, 4, N, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(fn=_abi.FN_TERNARY_TANH), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(fn=_abi.FN_LEAKY_RELU, out_store=T.I4), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(fn=_abi.FN_QUANTIZED_TANH, act_bits=8, out_store=T.I4), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(fn=_abi.FN_QUANTIZED_TANH, act_bits=4, out_store=T.BIN), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(out_store=T.T2), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(bn_inv=some.data_ptr()), y)[0] == EINVAL
    assert _forward_rc(w, xd, T.I4, 4, N, H, W, _epi(), xd)[0] == EINVAL          # y overlaps x
    # 2^31 output words: refused before any pointer is used
    rc, msg = _forward_rc(w, xd, T.I4, 4, 1 << 20, 64, 64, _epi(), y)
    assert rc == EUNSUP and "2^31" in msg
    # the int32 bound at its edge: 8-bit codes x 8-bit weights, 2x2 / 2 (one tap per output), Cin = 2^17 - 64 and 2^17
    for cin, want in (((1 << 17) - 64, 0), (1 << 17, EUNSUP)):
        big = _abi.TConvWeights(T.W_QUANT, 8, 1.0, torch.zeros((2, 2, 1, cin), device="cuda"), None, 2, True, T.I8)
        xb = torch.zeros((1, cin // 4), dtype=torch.int32, device="cuda")
        rc, msg = _forward_rc(big, xb, T.I8, 8, 1, 1, 1, _epi(), y)
        assert rc == want and (want == 0 or "int32" in msg), (cin, rc, msg)
        assert _forward_rc(big, xb, T.I8, 7, 1, 1, 1, _epi(), y)[0] == 0          # one bit less fits
    # N == 0: QNN_OK without a launch, null pointers allowed
    _forward_rc(*ok, _epi(), y)
    assert _forward_rc(w, None, T.I4, 4, 0, H, W, _epi(), None)[0] == 0
    # every refusal above left the kernel name alone
    assert _abi.last_kernel() == name
    # prepack
    k = dev(kernel)
    lib = _abi.load()

    def prepack(wkind=T.W_QUANT, wbits=4, kh=3, kw=3, F=8, C=8, stride=1, store=T.I4, kern=k):
        h = ctypes.c_void_p(None)
        rc = lib.qnn_tconv_prepack(wkind, wbits, 1.0, _abi.ptr(kern), kh, kw, F, C, None, stride, 1, store,
                                   _abi.stream_ptr(), ctypes.byref(h))
        msg = lib.qnn_last_error().decode()
        if rc == 0:
            lib.qnn_tconv_free(h)
        return rc, msg
    big = torch.zeros(9 * 9 * 8 * 8, device="cuda")
    assert prepack()[0] == 0 and prepack(kh=8, kw=8, kern=big)[0] == 0 and prepack(stride=4)[0] == 0
    for kwargs, field in ((dict(kh=9, kern=big), "kh"), (dict(kw=9, kern=big), "kw"), (dict(stride=5), "stride")):
        rc, msg = prepack(**kwargs)
        assert rc == EUNSUP and field in msg, (kwargs, rc, msg)
    assert prepack(stride=0)[0] == EINVAL and prepack(C=0)[0] == EINVAL and prepack(F=0)[0] == EINVAL
    assert prepack(kern=None)[0] == EINVAL and prepack(wbits=8)[0] == EINVAL and prepack(store=T.BIN)[0] == EINVAL
    assert prepack(wkind=T.W_FLOAT)[0] == EINVAL and prepack(wkind=7)[0] == EINVAL and prepack(store=3)[0] == EINVAL
    assert _abi.last_kernel() == name


# ---- capture ----------------------------------------------------------------------------------------------------------------
class _OneCall:
    """One qnn_tconv_forward call as the model engine.Pipelined captures: float32 images in, the codes as float32 out."""

    def __init__(self, c, w, bnd):
        self.c, self.w, self.bnd = c, w, bnd
        self.device = torch.device("cuda")

    def __call__(self, x):
        c = self.c
        N, H, W, C = x.shape
        xp = _abi.pack(x, C, _abi.FN_QUANTIZED_TANH, c["x_bits"], c["store"])
        y, Ho, Wo = _abi.tconv(self.w, xp, c["store"], c["x_bits"], N, H, W, self.bnd[0], self.bnd[1], c["fn"], c["act_bits"],
                               c["out_store"])
        return _abi.unpack(y, N * Ho * Wo, c["Cout"], c["out_store"], c["act_bits"]).view(N, Ho, Wo, c["Cout"])


def test_forward_call_is_captured_and_replayed_through_pipelined():
    from qnn_amd import engine
    c = T._case(T.I4, 64, 16, window=(2, 2), stride=2, map=(4, 4, 4))
    _, kernel, bias, bn = T.make_inputs(c)
    model = _OneCall(c, handle(c, kernel, bias), (dev(bn[0]), dev(bn[1])))
    rs = np.random.RandomState(5)
    B, H, W = c["map"]
    pipe = engine.Pipelined(model, lanes=2, batch_size=B)
    for _ in range(2):                       # the first call captures one graph per lane, the second only replays
        codes = T.random_codes(rs, (3 * B, H, W, 64), T.I4, 4)
        got = host(pipe(torch.from_numpy(T.values_of(codes, T.I4, 4)).cuda()))
        want = T.values_of(T.reference(dict(c, map=(3 * B, H, W)), codes, kernel, bias, bn), T.I4, 4)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert _abi.last_kernel() == "tconv_i4_mfma"


def test_forward_call_is_capturable():
    """No allocation, host read or synchronisation in qnn_tconv_forward (the matrix-pipe form): captured into a hipGraph
    and replayed on new input in the same buffers."""
    c = T._case(T.I4, 64, 16, window=(4, 4), stride=2, map=(3, 2, 15))
    x, kernel, bias, bn = T.make_inputs(c)
    N, H, W = c["map"]
    w = handle(c, kernel, bias)
    bnd = (dev(bn[0]), dev(bn[1]))
    xd = dev(T.encode(x, T.I4).reshape(N * H * W, -1))
    out = torch.zeros((N * 4 * H * W, T.words(T.I4, 16)), dtype=torch.int32, device="cuda")
    epi = _abi.make_epilogue(bnd[0], bnd[1], c["fn"], c["act_bits"], 1, T.I4, flags=0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _abi.tconv(w, xd, T.I4, 4, N, H, W, out_store=T.I4, out=out, epilogue=epi)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _abi.tconv(w, xd, T.I4, 4, N, H, W, out_store=T.I4, out=out, epilogue=epi)
    assert _abi.last_kernel() == "tconv_i4_mfma"
    x2 = T.make_inputs(c, seed=1)[0]
    xd.copy_(dev(T.encode(x2, T.I4).reshape(N * H * W, -1)))
    out.zero_()
    graph.replay()
    codes, _ = T.decode(host(out).reshape(N, 2 * H, 2 * W, -1), T.I4, 16)
    np.testing.assert_array_equal(codes, T.reference(c, x2, kernel, bias, bn))


# ---- the layer classes -----------------------------------------------------------------------------------------------------
LAYER_CASES = [
    (qnn_amd.Conv2DTranspose, {}, None, T.W_FLOAT, 0),
    (qnn_amd.Conv2DTranspose, {"strides": 2, "padding": "same", "use_bias": False}, None, T.W_FLOAT, 0),
    (qnn_amd.BinaryConv2DTranspose, {"padding": "same", "strides": 2}, "binary", T.W_BINARY, 1),
    (qnn_amd.QuantizedConv2DTranspose, {"nb": 4, "padding": "same", "strides": 3}, ("quantized", 4), T.W_QUANT, 4),
    (qnn_amd.QuantizedConv2DTranspose, {"nb": 4, "strides": 2}, None, T.W_QUANT, 4),
    (qnn_amd.TernaryConv2DTranspose, {"padding": "same", "strides": 2}, "ternary", T.W_TERNARY, 1),
]


@pytest.mark.parametrize("cls,kw,domain,wkind,wbits", LAYER_CASES)
def test_layer_classes(cls, kw, domain, wkind, wbits):
    rs = np.random.RandomState(5)
    N, H, W, C, F = 2, 3, 4, 9, 5
    layer = cls(F, (3, 3), input_domain=domain, **kw)
    layer.build((None, H, W, C))
    kernel = (rs.randint(-64, 65, (3, 3, F, C)) / 64.0).astype(np.float32)
    bias = (rs.randint(-8, 9, F) / 16.0).astype(np.float32)
    layer.set_weights([kernel, bias] if layer.use_bias else [kernel])
    np.testing.assert_array_equal(layer.get_weights()[0], kernel)
    if domain == "binary":
        x = rs.choice([-1.0, 1.0], (N, H, W, C)).astype(np.float32)
    elif domain == "ternary":
        x = rs.randint(-1, 2, (N, H, W, C)).astype(np.float32)
    elif domain is not None:
        x = (rs.randint(-8, 8, (N, H, W, C)) / 8.0).astype(np.float32)
    else:
        x = (rs.randint(-64, 65, (N, H, W, C)) / 64.0).astype(np.float32)
    q = T.quantize_weights(kernel, wkind, wbits)[0]
    np.testing.assert_array_equal(host(layer.quantized_kernel()), q)
    v = T.tconv_sum(x, q, layer.strides[0], layer.padding == "same", np.float64).astype(np.float32)
    want = T.chain(v, bias if layer.use_bias else None, None, T.FN_NONE, 0, T.F32)
    y = host(layer(torch.from_numpy(x).cuda()))
    assert y.shape == layer.compute_output_shape((N, H, W, C))
    np.testing.assert_array_equal(y.view(np.uint32), want.view(np.uint32))


# ---- the spec op on the engines ----------------------------------------------------------------------------------------------
def _conv_sum(x, w):
    """3x3 'same' stride-1 forward convolution of integer or dyadic values, HWIO kernel, exact in float64."""
    N, H, W, C = x.shape
    xp = np.zeros((N, H + 2, W + 2, C), np.float64)
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((N, H, W, w.shape[3]), np.float64)
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("nhwc,cf->nhwf", xp[:, ky:ky + H, kx:kx + W], w[ky, kx].astype(np.float64))
    return out


def unet_spec(skip=True, seed=0):
    """conv -> quantized_tanh -> maxpool -> conv -> act -> tconv 2x2 / 2 -> BN -> act -> [concat with the skip] -> conv ->
    globalavgpool -> dense, 4-bit throughout; the map being up-sampled has 64 channels."""
    rs = np.random.RandomState(90 + seed)
    k = lambda *shape: (rs.randint(-64, 65, shape) / 64.0).astype(np.float32)          # noqa: E731
    b = lambda n: (rs.randint(-8, 9, n) / 16.0).astype(np.float32)                     # noqa: E731
    conv = lambda cin, cout, **kw: dict({"op": "conv", "kind": "quantized", "nb": 4, "kernel": k(3, 3, cin, cout),  # noqa: E731
                                         "bias": b(cout), "strides": (1, 1), "padding": "same"}, **kw)
    act = lambda **kw: dict({"op": "act", "fn": "quantized_tanh", "nb": 4}, **kw)        # noqa: E731
    spec = [conv(3, 16), act(dst="skip"), {"op": "maxpool", "size": 2}, conv(16, 64, kernel=k(3, 3, 16, 64) / 4), act(),
            {"op": "tconv", "kind": "quantized", "nb": 4, "kernel": k(2, 2, 16, 64), "bias": b(16), "strides": (2, 2),
             "padding": "same", "H": 1.0},
            {"op": "bn", "eps": 0.0, "gamma": (2.0 ** rs.randint(-4, -1, 16)).astype(np.float32) * rs.choice([-1, 1], 16).astype(np.float32),
             "beta": b(16), "mean": np.zeros(16, np.float32), "var": np.ones(16, np.float32)},
            act(dst="up")]
    if skip:
        spec.append({"op": "concat", "srcs": ["up", "skip"]})
    spec += [conv(32 if skip else 16, 16, kernel=k(3, 3, 32 if skip else 16, 16) / 8), {"op": "globalavgpool"},
             {"op": "dense", "kind": "quantized", "nb": 4, "kernel": k(16, 10), "bias": b(10)}]
    return spec


def unet_reference(spec, x):
    f = np.float32
    ops = [op for op in spec if op["op"] in ("conv", "tconv", "bn", "dense")]
    c1, c2, tc, bn, c3, de = ops
    wq = lambda op: T.quantize_weights(op["kernel"], T.W_QUANT, 4)            # noqa: E731
    v = (_conv_sum(x, wq(c1)[0]).astype(f) + c1["bias"]).astype(f)               # float32 images: exact dyadic sums
    skip = T.qact_code(T.FN_QUANTIZED_TANH, v, 8).astype(np.int64)
    N, H, W, C = skip.shape
    pooled = skip.reshape(N, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))
    v = ((_conv_sum(pooled, wq(c2)[1]).astype(f) * f(2.0 ** -6)).astype(f) + c2["bias"]).astype(f)
    mid = T.qact_code(T.FN_QUANTIZED_TANH, v, 8).astype(np.int64)
    case = dict(store=T.I4, stride=2, same=True, wkind=T.W_QUANT, wbits=4, x_bits=4, fn=T.FN_QUANTIZED_TANH, act_bits=4,
                out_store=T.I4)
    up = T.reference(case, mid, tc["kernel"], tc["bias"], (bn["gamma"], bn["beta"]))
    cat = np.concatenate([up, skip], -1) if any(op["op"] == "concat" for op in spec) else up
    v = ((_conv_sum(cat, wq(c3)[1]).astype(f) * f(2.0 ** -6)).astype(f) + c3["bias"]).astype(f)
    avg = (v.astype(np.float64).sum(axis=(1, 2)) / (v.shape[1] * v.shape[2])).astype(f)      # dyadic, 64 pixels: exact
    return ((avg.astype(np.float64) @ wq(de)[0].astype(np.float64)).astype(f) + de["bias"]).astype(f)


def _images(seed=0):
    rs = np.random.RandomState(95 + seed)
    return (rs.randint(-16, 17, (3, 8, 8, 3)) / 16.0).astype(np.float32)


def test_encoder_decoder_on_graphmodel_keeps_codes_across_the_skip():
    from qnn_amd import engine, nets
    spec = unet_spec(skip=True)
    x = _images()
    want = unet_reference(spec, x)
    gm = engine.GraphModel(spec)
    gm.kernel_log = []
    y = host(gm(torch.from_numpy(x).cuda()))
    np.testing.assert_array_equal(y.view(np.uint32), want.view(np.uint32))
    log = gm.kernel_log
    assert "tconv_i4_mfma" in log, log
    t = log.index("tconv_i4_mfma")
    joins = [i for i, name in enumerate(log) if name.startswith("concat_")]
    assert joins and joins[0] > t and "unpack" not in log[t:joins[0] + 1], log
    assert isinstance(nets.Model(None, spec).engine, engine.GraphModel)
    for cls in (engine.FusedModel, engine.ResidualFusedModel):
        with pytest.raises(_abi.NotFusable):
            cls(spec)
    with pytest.raises(_abi.NotFusable, match="tconv"):
        engine.FusedModel(unet_spec(skip=False))


def test_decoder_chain_on_layermodel_and_graphmodel():
    """LayerModel reads one tensor per op and declines a concat, so it runs the same network without the skip."""
    from qnn_amd import engine, nets
    spec = unet_spec(skip=False)
    x = _images(1)
    want = unet_reference(spec, x)
    xd = torch.from_numpy(x).cuda()
    np.testing.assert_array_equal(host(engine.LayerModel(spec)(xd)).view(np.uint32), want.view(np.uint32))
    gm = engine.GraphModel(spec)
    gm.kernel_log = []
    np.testing.assert_array_equal(host(gm(xd)).view(np.uint32), want.view(np.uint32))
    assert "tconv_i4_mfma" in gm.kernel_log and "unpack" not in gm.kernel_log
    assert isinstance(nets.Model(None, spec).engine, engine.GraphModel)
    with pytest.raises(_abi.NotFusable, match="concat"):
        engine.LayerModel(unet_spec(skip=True))


def test_float_tconv_and_a_batch_scaled_activation_in_front():
    from qnn_amd import engine
    rs = np.random.RandomState(70)
    k = (rs.randint(-64, 65, (3, 3, 5, 3)) / 64.0).astype(np.float32)
    b = (rs.randint(-8, 9, 5) / 16.0).astype(np.float32)
    tc = {"op": "tconv", "kind": "float", "kernel": k, "bias": b, "strides": (2, 2), "padding": "valid", "H": 1.0}
    x = (rs.randint(-64, 65, (2, 3, 4, 3)) / 64.0).astype(np.float32)
    c = dict(store=T.F32, stride=2, same=False, wkind=T.W_FLOAT, fn=T.FN_NONE, out_store=T.F32)
    want = T.reference(c, x, k, b, None)
    for cls in (engine.GraphModel, engine.LayerModel):
        np.testing.assert_array_equal(host(cls([tc])(torch.from_numpy(x).cuda())).view(np.uint32), want.view(np.uint32))
    spec = [{"op": "act", "fn": "quantized_maxrelu", "nb": 4}, dict(tc, kind="quantized", nb=4)]
    xd = torch.from_numpy(x).cuda()
    plain, scaled = engine.GraphModel(spec), engine.GraphModel(spec, scaled_codes=True)
    scaled.kernel_log = []
    np.testing.assert_array_equal(host(plain(xd)), host(scaled(xd)))
    assert scaled.kernel_log == ["tconv_f32"]
