"""The grouped convolution on the GPU (include/qnn_abi_gconv.h, csrc/qnn_gconv.hip) against the numpy reference of
gconv_cases.py, bit for bit, with the kernel name asserted in every case: the plain form on every store with group edges
inside words, every window, stride, dilation, padding, weight kind and epilogue, the input's spare bits set and pointers
moved off their 16-byte alignment; the cross-checks against qnn_conv2d_forward (g = 1) and qnn_depthwise_forward
(g = Cin); the matrix-pipe form against the reference and against the plain form, on one and on several wave tasks per
image; the plain form beyond one workgroup; the route's edges; every refusal; capture; the layer classes; the spec op on
the engines."""
import ctypes

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi

import gconv_cases as G

pytestmark = pytest.mark.gpu
ENTRIES = _abi.EXPORTS_GCONV              # read at import: without the entries nothing below means anything
FILL = 0x5A5A5A5A
NAMES = {G.F32: "f32", G.BIN: "bin", G.T2: "t2", G.I4: "i4", G.I8: "i8"}


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
    return _abi.GConvWeights(c["wkind"], c["wbits"], 1.0, dev(kernel), dev(bias) if bias is not None else None, c["groups"],
                             c["stride"], c["same"], c["store"] if store is None else store, dilation=c["dil"])


def expected_name(c):
    if c["store"] in (G.I4, G.I8):
        return "gconv_%s_%s" % (NAMES[c["store"]], "mfma" if G.takes_mfma(c) else "plain")
    return "gconv_" + NAMES[c["store"]]


def run_case(c, inputs=None, seed=0, w=None, check_weights=True, misalign_y=False, guard=0):
    """One forward call of case `c` compared with the reference; returns the decoded output (values or codes).  `guard`:
    that many pixels' words of FILL lie behind an aligned, packed output and must still be FILL after the call."""
    x, kernel, bias, bn = inputs if inputs is not None else G.make_inputs(c, seed)
    N, H, W = c["map"]
    cout = c["Cout"]
    want = G.reference(c, x, kernel, bias, bn)
    w = handle(c, kernel, bias) if w is None else w
    if check_weights:
        np.testing.assert_array_equal(host(w.dequant()).view(np.uint32),
                                      G.quantize_weights(kernel, c["wkind"], c["wbits"])[0].view(np.uint32))
    if c["store"] == G.F32:
        xd = dev(x, c["misalign"])
    else:
        xd = dev(G.encode(x, c["store"], spare=np.random.RandomState(7)).reshape(N * H * W, -1), c["misalign"])
    Ho, Wo = want.shape[1:3]
    assert (Ho, Wo) == w.out_hw(H, W)
    if c["out_store"] == G.F32:
        shape, dt = (N, Ho, Wo, cout), np.float32
    else:
        shape, dt = (N * Ho * Wo, G.words(c["out_store"], cout)), np.uint32
    if guard:
        assert dt == np.uint32 and not (c["misalign"] or misalign_y)
        behind = dev(np.full((shape[0] + guard, shape[1]), FILL, np.uint32))
        out = behind[:shape[0]]
    else:
        out = dev(np.full(shape, FILL, np.uint32).view(dt), c["misalign"] or misalign_y)
    bnd = (dev(bn[0]), dev(bn[1])) if bn is not None else (None, None)
    y, ho, wo = _abi.gconv(w, xd, c["store"], c["x_bits"], N, H, W, bnd[0], bnd[1], c["fn"], c["act_bits"], c["out_store"],
                           out=out)
    assert _abi.last_kernel() == expected_name(dict(c, misalign=c["misalign"] or misalign_y))
    assert (ho, wo) == (Ho, Wo)
    got = host(y)
    if guard:
        assert (host(behind)[shape[0]:] == FILL).all(), "words behind the output were written"
    if c["out_store"] == G.F32:
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        return got
    codes, spare = G.decode(got.reshape(N, Ho, Wo, -1), c["out_store"], cout)
    np.testing.assert_array_equal(codes, want)
    assert not spare.any(), "spare bits of the last word are not zero"
    return codes


def run_all(cases, **kw):
    """run_case on every case of a group (a dozen tiny calls); a failure names its case."""
    assert cases
    for c in cases:
        try:
            run_case(c, **kw)
        except AssertionError as e:
            raise AssertionError("case %s: %s" % (G.case_id(c), e)) from e


# ---- the plain form --------------------------------------------------------------------------------------------------------
# The case tables of gconv_cases.py are walked in groups, one test per (store, group shape) or (store, constants): every
# case runs and is compared on its own, with the kernel name asserted (run_case).
@pytest.mark.parametrize("store,shape", [(s_, sh) for s_ in G.STORES for sh in G.GROUP_SHAPES[s_]],
                         ids=lambda v: NAMES[v] if isinstance(v, int) else "%dx%d" % v)
def test_plain_form(store, shape):
    """g in {1, 2, 3, 4} x three geometries of the round robin for one (Cg, Fg) on one store."""
    cases = [c for c in G.plain_cases() if c["store"] == store and (c["Cg"], c["Fg"]) == shape]
    assert {c["groups"] for c in cases} == {1, 2, 3, 4} and len(cases) == 12
    run_all(cases)


@pytest.mark.parametrize("store", [G.I4, G.I8, G.T2, G.F32], ids=lambda v: NAMES[v])
def test_weight_kinds(store):
    run_all([c for c in G.weight_cases() if c["store"] == store])


EPILOGUE_HOST_STORES = [s_ for s_ in G.STORES for _ in range(2)]          # test_epilogues: store x (bias, bn)


@pytest.mark.parametrize("bias,bn", [(True, True), (False, False)])
@pytest.mark.parametrize("store", G.STORES, ids=lambda v: NAMES[v])
def test_epilogues(store, bias, bn):
    """Every fn to every legal out_store on one input store."""
    cases = [c for c in G.epilogue_cases() if c["store"] == store and (c["bias"], c["bn"]) == (bias, bn)]
    assert len(cases) == len(G._fn_pairs())
    import test_gpu_sideconv_grid as grid
    try:
        run_all(cases)
    finally:
        # on exact ties, zeros and clip edges: the groups of sideconv_grid_cases.py that this id carries (its own input store)
        grid.run_hosted("gc", EPILOGUE_HOST_STORES, 2 * G.STORES.index(store) + (0 if bias else 1))


def test_aligned_and_misaligned_agree():
    """4-byte-aligned pointers take V = 1, 16-byte-aligned ones V = 4 where the words per pixel divide by 4."""
    for c in (G._case(G.F32, 3, 4, 2), G._case(G.BIN, 33, 64, 2), G._case(G.T2, 33, 16, 2), G._case(G.I4, 3, 8, 4),
              G._case(G.I8, 3, 8, 2), G._case(G.I4, 3, 5, 3)):
        a = run_case(c)
        b = run_case(dict(c, misalign=True))
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                      b.view(np.uint32) if b.dtype == np.float32 else b)
    # the same on more than 256 items (the plain case of G.multitask_cases()): blockIdx.x > 0 in the item decode
    cases = [c for c in G.multitask_cases() if not G.takes_mfma(c)]
    assert [c["misalign"] for c in cases] == [False, True]
    a, b = (run_multitask(c) for c in cases)
    assert _abi.last_kernel() == "gconv_i4_plain"
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- cross-checks against the existing entries ------------------------------------------------------------------------------
@pytest.mark.parametrize("store,cin,cout", [(G.I4, 9, 5), (G.I8, 5, 8), (G.BIN, 33, 5), (G.T2, 33, 5)])
def test_one_group_equals_conv2d_forward(store, cin, cout):
    c = G._case(store, cin, cout, 1)
    x, kernel, bias, bn = G.make_inputs(c)
    N, H, W = c["map"]
    codes = run_case(c, (x, kernel, bias, bn))
    w = _abi.Weights(c["wkind"], c["wbits"], 1.0, dev(kernel), dev(bias), 1, True, store)
    xd = dev(G.encode(x, store).reshape(N * H * W, -1))
    y, _, _ = _abi.conv2d(w, xd, store, c["x_bits"], N, H, W, dev(bn[0]), dev(bn[1]), c["fn"], c["act_bits"], 1, c["out_store"])
    got, _ = G.decode(host(y).reshape(N, H, W, -1), c["out_store"], cout)
    np.testing.assert_array_equal(got, codes)


@pytest.mark.parametrize("store,C,M", [(G.I4, 9, 1), (G.I4, 16, 2), (G.I8, 5, 2), (G.BIN, 33, 1), (G.T2, 33, 2)])
def test_groups_equal_channels_equals_depthwise_forward(store, C, M):
    c = G._case(store, 1, M, C)
    x, kernel, bias, bn = G.make_inputs(c)
    N, H, W = c["map"]
    codes = run_case(c, (x, kernel, bias, bn))
    w = _abi.DepthwiseWeights(c["wkind"], c["wbits"], 1.0, dev(kernel.reshape(3, 3, C, M)), dev(bias), 1, True, store)
    xd = dev(G.encode(x, store).reshape(N * H * W, -1))
    y, _, _ = _abi.depthwise(w, xd, store, c["x_bits"], N, H, W, dev(bn[0]), dev(bn[1]), c["fn"], c["act_bits"], c["out_store"])
    got, _ = G.decode(host(y).reshape(N, H, W, -1), c["out_store"], C * M)
    np.testing.assert_array_equal(got, codes)


# ---- the matrix-pipe form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.MFMA_SHAPES, ids=lambda v: "%dx%dg%d" % v)
@pytest.mark.parametrize("store", [G.I4, G.I8], ids=lambda v: NAMES[v])
def test_matrix_pipe_equals_reference_and_plain_form(store, shape):
    """One (Cg, Fg, g) on one store at its three geometries: against the reference and against the plain form.  The shapes of
    G.MULTITASK_SHAPES then run their maps of several wave tasks per image."""
    cases = [c for c in G.mfma_cases() if c["store"] == store and (c["Cg"], c["Fg"], c["groups"]) == shape]
    assert len(cases) == 3
    for c in cases:
        c = dict(c, act_bits=4)
        inputs = G.make_inputs(c)
        w = handle(c, inputs[1], inputs[2])
        fast = run_case(c, inputs, w=w)
        assert _abi.last_kernel() == "gconv_%s_mfma" % NAMES[store], G.case_id(c)
        off = run_case(dict(c, misalign=True), inputs, w=w, check_weights=False)
        assert _abi.last_kernel() == "gconv_%s_plain" % NAMES[store], G.case_id(c)
        np.testing.assert_array_equal(fast, off, err_msg=G.case_id(c))
    _several_wave_tasks_per_image(store, shape)


def run_multitask(c, **kw):
    """run_case on a case of G.multitask_cases() with its own seed; on top of it, no word of the output is the pattern
    laid under it (test_gconv_cpu.py: no expected word is)."""
    try:
        got = run_case(c, G.make_inputs(c, c["seed"]), **kw)
        words = got.view(np.uint32) if c["out_store"] == G.F32 else G.encode(got, c["out_store"])
        assert not (words == FILL).any(), "an output word was not written"
    except AssertionError as e:
        raise AssertionError("case %s: %s" % (G.case_id(c), e)) from e
    return got


def _several_wave_tasks_per_image(store, shape):
    """The cases of G.multitask_cases() on one (store, shape): g0 > 0 with n > 0, ragged and empty groups in a later task,
    the int4 exchange with one valid member, a partly filled last workgroup -- against the reference and against the plain
    form.  Every case runs; the failures are reported together, each under its case id."""
    cases = [c for c in G.multitask_cases() if G.takes_mfma(c) and (c["store"], c["Cg"], c["Fg"], c["groups"]) == (store,) + shape]
    assert len(cases) == (0 if shape not in G.MULTITASK_SHAPES else 5 if (store, shape) == (G.I4, (4, 4, 4)) else 4)
    failures = []
    for c in cases:
        try:
            w = handle(c, *G.make_inputs(c, c["seed"])[1:3])
            fast = run_multitask(c, w=w, guard=16 * G.K_PG)      # a task's pixels beyond the last image would land there
            assert _abi.last_kernel() == "gconv_%s_mfma" % NAMES[store], G.case_id(c)
            off = run_multitask(dict(c, misalign=True), w=w, check_weights=False)
            assert _abi.last_kernel() == "gconv_%s_plain" % NAMES[store], G.case_id(c)
            np.testing.assert_array_equal(fast, off, err_msg=G.case_id(c))
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "%d of %d multitask cases:\n%s" % (len(failures), len(cases), "\n".join(failures))


@pytest.mark.parametrize("store", [G.I4, G.I8])
@pytest.mark.parametrize("Cg,Fg,g,window", [(4, 4, 4, (3, 3)), (128, 16, 2, (3, 3)), (16, 16, 2, (7, 7)), (2, 1, 16, (5, 5))])
def test_matrix_pipe_largest_sums(store, Cg, Fg, g, window):
    """Inputs and weights all at the most negative code: the largest |acc| a shape can reach, through both forms."""
    c = G._case(store, Cg, Fg, g, window=window, map=(1, 5, 5), extreme=True, bn=False, bias=False,
                fn=G.FN_NONE, act_bits=0, out_store=G.F32)
    run_case(c)                              # float32 output: the plain form, the sum itself visible
    c = G._case(store, Cg, Fg, g, window=window, map=(1, 5, 5), extreme=True)
    inputs = G.make_inputs(c)
    bn = (np.full(c["Cout"], 2.0 ** -10, np.float32), np.zeros(c["Cout"], np.float32))
    inputs = inputs[:3] + (bn,)
    fast = run_case(c, inputs)
    assert _abi.last_kernel() == "gconv_%s_mfma" % NAMES[store]
    np.testing.assert_array_equal(fast, run_case(dict(c, misalign=True), inputs))


@pytest.mark.parametrize("store,x_bits,wkind,wbits", [
    (G.I4, 2, G.W_QUANT, 4), (G.I4, 4, G.W_QUANT, 2), (G.I4, 4, G.W_BINARY, 1), (G.I4, 2, G.W_TERNARY, 1),
    (G.I8, 3, G.W_QUANT, 8), (G.I8, 8, G.W_QUANT, 4), (G.I8, 8, G.W_BINARY, 1), (G.I8, 3, G.W_TERNARY, 1)])
def test_matrix_pipe_widths_and_weight_kinds(store, x_bits, wkind, wbits):
    c = G._case(store, 8, 8, 4, map=(3, 5, 5), x_bits=x_bits, wkind=wkind, wbits=wbits, act_bits=4)
    run_case(c)
    assert _abi.last_kernel() == "gconv_%s_mfma" % NAMES[store]


@pytest.mark.parametrize("store", [G.I4, G.I8])
@pytest.mark.parametrize("bias,bn", [(True, True), (False, False), (True, False), (False, True)])
def test_matrix_pipe_epilogues(store, bias, bn):
    for fn, act_bits in ((G.FN_BINARY_TANH, 0), (G.FN_QUANTIZED_TANH, 4), (G.FN_QUANTIZED_TANH, 2), (G.FN_QUANTIZED_RELU, 4),
                         (G.FN_QUANTIZED_LEAKYRELU, 3)):
        c = G._case(store, 4, 4, 8, map=(3, 5, 5), fn=fn, act_bits=act_bits, bias=bias, bn=bn)
        run_all([c])
        assert _abi.last_kernel() == "gconv_%s_mfma" % NAMES[store], G.case_id(c)


@pytest.mark.parametrize("c", G.boundary_cases(), ids=G.case_id)
def test_route_boundaries_take_the_plain_form(c):
    run_case(c)
    assert _abi.last_kernel() == "gconv_%s_plain" % NAMES[c["store"]]


@pytest.mark.parametrize("store", [G.I4, G.I8])
def test_other_out_store_and_misaligned_y_take_the_plain_form(store):
    c = G._case(store, 4, 4, 4, act_bits=4)
    inputs = G.make_inputs(c)
    fast = run_case(c, inputs)
    assert _abi.last_kernel() == "gconv_%s_mfma" % NAMES[store]
    other = run_case(dict(c, out_store=G.I8 if store == G.I4 else G.I4), inputs)
    assert _abi.last_kernel() == "gconv_%s_plain" % NAMES[store]
    np.testing.assert_array_equal(fast, other)
    moved = run_case(c, inputs, misalign_y=True)
    assert _abi.last_kernel() == "gconv_%s_plain" % NAMES[store]
    np.testing.assert_array_equal(fast, moved)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _epi(**kw):
    e = _abi.make_epilogue(None, None, _abi.FN_NONE, 0, 1, _abi.STORE_F32, flags=0)
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _forward_rc(w, x, x_store, x_bits, N, H, W, epi, y):
    lib = _abi.load()
    rc = lib.qnn_gconv_forward(w.handle if w is not None else None, _abi.ptr(x), x_store, x_bits, N, H, W,
                               ctypes.byref(epi), _abi.ptr(y), _abi.stream_ptr())
    return rc, lib.qnn_last_error().decode()


def test_refusals_and_empty_batch():
    EINVAL, EUNSUP = -1, -2
    c = G._case(G.I4, 4, 4, 2)
    x, kernel, bias, bn = G.make_inputs(c)
    N, H, W = c["map"]
    w = handle(c, kernel, bias)
    xd = dev(G.encode(x, G.I4).reshape(N * H * W, -1))
    y = torch.full((N, H, W, 8), 7.0, dtype=torch.float32, device="cuda")
    some = torch.zeros(64, dtype=torch.float32, device="cuda")
    ok = (w, xd, G.I4, 4, N, H, W)
    assert _forward_rc(*ok, _epi(), y)[0] == 0
    name = _abi.last_kernel()
    assert name == "gconv_i4_plain"
    y.fill_(7.0)                             # the poison: no refused call may write y
    for field, value in (("pool", 2), ("res", some.data_ptr()), ("fold", some.data_ptr()), ("proj", some.data_ptr()),
                         ("trick_s", 2.0), ("flags", 1)):
        rc, msg = _forward_rc(*ok, _epi(**{field: value}), y)
        assert rc == EUNSUP and field in msg, (field, rc, msg)
    for xs in (_abi.STORE_U8, _abi.STORE_F32_IMAGE, _abi.STORE_F32_UNIT):
        rc, msg = _forward_rc(w, xd, xs, 4, N, H, W, _epi(), y)
        assert rc == EUNSUP and "x_store" in msg
    for fn in _abi.MAXACT_FNS:
        rc, msg = _forward_rc(*ok, _epi(fn=fn, act_bits=4), y)
        assert rc == EUNSUP and "fn" in msg
    # QNN_EINVAL
    assert _forward_rc(w, None, G.I4, 4, N, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, G.I4, 4, N, H, W, _epi(), None)[0] == EINVAL
    assert _forward_rc(None, xd, G.I4, 4, N, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, G.I4, 4, -1, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, G.I4, 4, N, 0, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, G.I8, 4, N, H, W, _epi(), y)[0] == EINVAL          # not the handle's store
    assert _forward_rc(w, xd, G.I4, 5, N, H, W, _epi(), y)[0] == EINVAL          # x_bits beyond the store
    assert _forward_rc(w, xd, G.I4, 0, N, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(w, xd, 3, 4, N, H, W, _epi(), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(fn=_abi.FN_TERNARY_TANH), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(fn=_abi.FN_LEAKY_RELU, out_store=G.I4), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(fn=_abi.FN_QUANTIZED_TANH, act_bits=8, out_store=G.I4), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(fn=_abi.FN_QUANTIZED_TANH, act_bits=4, out_store=G.BIN), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(out_store=G.T2), y)[0] == EINVAL
    assert _forward_rc(*ok, _epi(bn_inv=some.data_ptr()), y)[0] == EINVAL
    assert _forward_rc(w, xd, G.I4, 4, N, H, W, _epi(), xd)[0] == EINVAL          # y overlaps x
    # an empty output: a 'valid' 3x3 window on a 2x2 image
    wv = handle(dict(c, same=False), kernel, bias)
    rc, msg = _forward_rc(wv, xd, G.I4, 4, 1, 2, 2, _epi(), y)
    assert rc == EINVAL and "empty" in msg
    # 2^31 output words: refused before any pointer is used
    rc, msg = _forward_rc(w, xd, G.I4, 4, 1 << 20, 64, 64, _epi(), y)
    assert rc == EUNSUP and "2^31" in msg
    # the int32 bound: 7x7, Cg = 4096, 8-bit codes x 8-bit weights on a 1x1 image
    assert G.int32_refused(7, 7, 4096, 8, 7) and not G.int32_refused(7, 7, 4096, 7, 7)
    big = _abi.GConvWeights(G.W_QUANT, 8, 1.0, torch.zeros((7, 7, 4096, 16), device="cuda"), None, 1, 1, True, G.I8)
    xb = torch.zeros((1, 4096 // 4), dtype=torch.int32, device="cuda")
    rc, msg = _forward_rc(big, xb, G.I8, 8, 1, 1, 1, _epi(), y)
    assert rc == EUNSUP and "int32" in msg, (rc, msg)
    assert host(y).min() == 7.0 and host(y).max() == 7.0, "a refused call wrote y"
    assert _forward_rc(big, xb, G.I8, 7, 1, 1, 1, _epi(), y)[0] == 0              # one bit less fits
    # N == 0: QNN_OK without a launch, null pointers allowed
    _forward_rc(*ok, _epi(), y)
    y.fill_(7.0)
    assert _forward_rc(w, None, G.I4, 4, 0, H, W, _epi(), None)[0] == 0
    assert _forward_rc(*ok[:4], 0, H, W, _epi(), y)[0] == 0
    assert host(y).min() == 7.0 and host(y).max() == 7.0
    assert _abi.last_kernel() == name
    # prepack
    k = dev(kernel)
    lib = _abi.load()

    def prepack(wkind=G.W_QUANT, wbits=4, kh=3, kw=3, C=8, F=8, groups=2, stride=1, dil=(1, 1), store=G.I4, kern=k):
        h = ctypes.c_void_p(None)
        rc = lib.qnn_gconv_prepack(wkind, wbits, 1.0, _abi.ptr(kern), kh, kw, C, F, groups, None, stride, 1, dil[0], dil[1],
                                   store, _abi.stream_ptr(), ctypes.byref(h))
        msg = lib.qnn_last_error().decode()
        if rc == 0:
            lib.qnn_gconv_free(h)
        return rc, msg
    big = torch.zeros(8 * 8 * 8 * 8, device="cuda")
    assert prepack()[0] == 0 and prepack(kh=7, kw=7, kern=big)[0] == 0 and prepack(stride=2)[0] == 0
    assert prepack(dil=(64, 64))[0] == 0 and prepack(groups=8)[0] == 0 and prepack(groups=1, kern=big)[0] == 0
    for kwargs, field in ((dict(kh=8, kern=big), "kh"), (dict(kw=8, kern=big), "kw"), (dict(stride=3), "stride"),
                          (dict(dil=(65, 1)), "dilation"), (dict(dil=(2, 2), stride=2), "dilation")):
        rc, msg = prepack(**kwargs)
        assert rc == EUNSUP and field in msg, (kwargs, rc, msg)
    assert prepack(stride=0)[0] == EINVAL and prepack(C=0)[0] == EINVAL and prepack(F=0)[0] == EINVAL
    assert prepack(dil=(0, 1))[0] == EINVAL and prepack(groups=0)[0] == EINVAL
    for kwargs in (dict(groups=3), dict(C=9, groups=3), dict(F=9, groups=3), dict(groups=16)):
        rc, msg = prepack(**kwargs)
        assert rc == EINVAL and "groups" in msg, (kwargs, rc, msg)
    assert prepack(kern=None)[0] == EINVAL and prepack(wbits=8)[0] == EINVAL and prepack(store=G.BIN)[0] == EINVAL
    assert prepack(wkind=G.W_FLOAT)[0] == EINVAL and prepack(wkind=7)[0] == EINVAL and prepack(store=3)[0] == EINVAL
    assert _abi.last_kernel() == name


# ---- capture ----------------------------------------------------------------------------------------------------------------
class _OneCall:
    """One qnn_gconv_forward call as the model engine.Pipelined captures: float32 images in, the codes as float32 out."""

    def __init__(self, c, w, bnd):
        self.c, self.w, self.bnd = c, w, bnd
        self.device = torch.device("cuda")

    def __call__(self, x):
        c = self.c
        N, H, W, C = x.shape
        xp = _abi.pack(x, C, _abi.FN_QUANTIZED_TANH, c["x_bits"], c["store"])
        y, Ho, Wo = _abi.gconv(self.w, xp, c["store"], c["x_bits"], N, H, W, self.bnd[0], self.bnd[1], c["fn"], c["act_bits"],
                               c["out_store"])
        return _abi.unpack(y, N * Ho * Wo, c["Cout"], c["out_store"], c["act_bits"]).view(N, Ho, Wo, c["Cout"])


def test_forward_call_is_captured_and_replayed_through_pipelined():
    from qnn_amd import engine
    c = G._case(G.I4, 4, 4, 4, map=(4, 4, 4))
    _, kernel, bias, bn = G.make_inputs(c)
    model = _OneCall(c, handle(c, kernel, bias), (dev(bn[0]), dev(bn[1])))
    rs = np.random.RandomState(5)
    B, H, W = c["map"]
    pipe = engine.Pipelined(model, lanes=2, batch_size=B)
    for _ in range(2):                       # the first call captures one graph per lane, the second only replays
        codes = G.random_codes(rs, (3 * B, H, W, 16), G.I4, 4)
        got = host(pipe(torch.from_numpy(G.values_of(codes, G.I4, 4)).cuda()))
        want = G.values_of(G.reference(dict(c, map=(3 * B, H, W)), codes, kernel, bias, bn), G.I4, 4)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert _abi.last_kernel() == "gconv_i4_mfma"


# ---- the layer classes -----------------------------------------------------------------------------------------------------
LAYER_CASES = [
    (qnn_amd.GroupedConv2D, {"groups": 3}, None, G.W_FLOAT, 0),
    (qnn_amd.GroupedConv2D, {"groups": 3, "strides": 2, "padding": "same", "use_bias": False}, None, G.W_FLOAT, 0),
    (qnn_amd.BinaryGroupedConv2D, {"groups": 3, "padding": "same"}, "binary", G.W_BINARY, 1),
    (qnn_amd.BinaryGroupedConv2D, {"groups": 3, "padding": "same"}, ("binary_tanh",), G.W_BINARY, 1),
    (qnn_amd.QuantizedGroupedConv2D, {"groups": 3, "nb": 4, "padding": "same", "dilation_rate": 2}, ("quantized", 4), G.W_QUANT, 4),
    (qnn_amd.QuantizedGroupedConv2D, {"groups": 3, "nb": 4, "padding": "same"}, ("quantized_tanh", 4), G.W_QUANT, 4),
    (qnn_amd.QuantizedGroupedConv2D, {"groups": 1, "nb": 4, "strides": 2}, None, G.W_QUANT, 4),
    (qnn_amd.TernaryGroupedConv2D, {"groups": 3, "padding": "same"}, "ternary", G.W_TERNARY, 1),
]


@pytest.mark.parametrize("cls,kw,domain,wkind,wbits", LAYER_CASES)
def test_layer_classes(cls, kw, domain, wkind, wbits):
    rs = np.random.RandomState(5)
    N, H, W, C, F = 2, 5, 4, 9, 6
    g = kw["groups"]
    layer = cls(F, (3, 3), input_domain=domain, **kw)
    layer.build((None, H, W, C))
    kernel = (rs.randint(-64, 65, (3, 3, C // g, F)) / 64.0).astype(np.float32)
    bias = (rs.randint(-8, 9, F) / 16.0).astype(np.float32)
    layer.set_weights([kernel, bias] if layer.use_bias else [kernel])
    np.testing.assert_array_equal(layer.get_weights()[0], kernel)
    if domain == "binary":
        x = rs.choice([-1.0, 1.0], (N, H, W, C)).astype(np.float32)
    elif domain == "ternary":
        x = rs.randint(-1, 2, (N, H, W, C)).astype(np.float32)
    elif domain == ("quantized", 4):
        x = (rs.randint(-8, 8, (N, H, W, C)) / 8.0).astype(np.float32)
    else:
        x = (rs.randint(-96, 97, (N, H, W, C)) / 64.0).astype(np.float32)
    seen = x                                 # what the contraction sees: a clip named by the domain is applied on load
    if domain == ("binary_tanh",):
        seen = G.chain(x, None, None, G.FN_BINARY_TANH, 0, G.F32)
    elif domain == ("quantized_tanh", 4):
        seen = G.chain(x, None, None, G.FN_QUANTIZED_TANH, 4, G.F32)
    q = G.quantize_weights(kernel, wkind, wbits)[0]
    np.testing.assert_array_equal(host(layer.quantized_kernel()), q)
    v = G.gconv_sum(seen, q, g, layer.strides[0], layer.padding == "same", layer.dilation_rate, np.float64).astype(np.float32)
    want = G.chain(v, bias if layer.use_bias else None, None, G.FN_NONE, 0, G.F32)
    y = host(layer(torch.from_numpy(x).cuda()))
    assert y.shape == layer.compute_output_shape((N, H, W, C))
    np.testing.assert_array_equal(y.view(np.uint32), want.view(np.uint32))


# ---- the spec op on the engines ----------------------------------------------------------------------------------------------
def resnext_spec(skip=True, seed=0):
    """act -> 1x1 conv -> BN -> quantized_tanh(4) -> 3x3 gconv g = 4 (16 -> 16) -> BN -> act -> 1x1 conv -> [add the skip] ->
    act, 4-bit throughout."""
    rs = np.random.RandomState(190 + seed)
    k = lambda *shape: (rs.randint(-64, 65, shape) / 64.0).astype(np.float32)          # noqa: E731
    b = lambda n: (rs.randint(-8, 9, n) / 16.0).astype(np.float32)                     # noqa: E731
    bn = lambda n: {"op": "bn", "eps": 0.0, "gamma": (2.0 ** rs.randint(-3, 0, n)).astype(np.float32) *   # noqa: E731
                    rs.choice([-1, 1], n).astype(np.float32), "beta": b(n), "mean": np.zeros(n, np.float32),
                    "var": np.ones(n, np.float32)}
    act = lambda **kw: dict({"op": "act", "fn": "quantized_tanh", "nb": 4}, **kw)        # noqa: E731
    conv = lambda cin, cout: {"op": "conv", "kind": "quantized", "nb": 4, "kernel": k(1, 1, cin, cout), "bias": b(cout),  # noqa: E731
                              "strides": (1, 1), "padding": "same"}
    spec = [act(dst="x0"), conv(16, 16), bn(16), act(),
            {"op": "gconv", "kind": "quantized", "nb": 4, "kernel": k(3, 3, 4, 16), "bias": b(16), "groups": 4,
             "strides": (1, 1), "padding": "same", "dilation": (1, 1), "H": 1.0, "klm": np.float32(1.0)},
            bn(16), act(), dict(conv(16, 16), dst="c2")]
    if skip:
        spec.append({"op": "add", "a": "c2", "b": "x0"})
    spec.append(act())
    return spec


def resnext_reference(spec, x):
    f = np.float32
    c1, b1, gc, b2, c2 = [op for op in spec if op["op"] in ("conv", "gconv", "bn")]
    qt = lambda v: G.qact_code(G.FN_QUANTIZED_TANH, v, 8).astype(np.int64)             # noqa: E731

    def pointwise(codes, op):
        _, wcode, _ = G.quantize_weights(op["kernel"], G.W_QUANT, 4)
        acc = np.einsum("nhwc,cf->nhwf", codes, wcode[0, 0])
        return ((acc.astype(f) * f(2.0 ** -6)).astype(f) + op["bias"]).astype(f)
    x0 = qt(x)
    v = pointwise(x0, c1)
    a1 = qt((v * b1["gamma"] + b1["beta"]).astype(f))
    case = dict(store=G.I4, groups=4, stride=1, same=True, dil=(1, 1), wkind=G.W_QUANT, wbits=4, x_bits=4,
                fn=G.FN_QUANTIZED_TANH, act_bits=4, out_store=G.I4)
    a2 = G.reference(case, a1, gc["kernel"], gc["bias"], (b2["gamma"], b2["beta"]))
    v = pointwise(a2, c2)
    if any(op["op"] == "add" for op in spec):
        v = (G.values_of(x0, G.I4, 4) + v).astype(f)
    return G.values_of(qt(v), G.I4, 4)


def _features(seed=0):
    rs = np.random.RandomState(195 + seed)
    return (rs.randint(-24, 25, (3, 5, 5, 16)) / 16.0).astype(np.float32)


def _record_conv_stores(monkeypatch):
    """The x_store of every _abi.conv2d call from here on (GraphModel's contractions do not write the kernel log)."""
    stores, real = [], _abi.conv2d

    def conv2d(w, x, x_store, *args, **kw):
        stores.append(x_store)
        return real(w, x, x_store, *args, **kw)
    monkeypatch.setattr(_abi, "conv2d", conv2d)
    return stores


def test_resnext_block_on_graphmodel_keeps_codes(monkeypatch):
    from qnn_amd import engine, nets
    spec = resnext_spec(skip=True)
    x = _features()
    want = resnext_reference(spec, x)
    gm = engine.GraphModel(spec)
    gm.kernel_log = []
    conv_stores = _record_conv_stores(monkeypatch)
    y = host(gm(torch.from_numpy(x).cuda()))
    np.testing.assert_array_equal(y.view(np.uint32), want.view(np.uint32))
    log = gm.kernel_log
    # the plan: the producer's clip is packed once, the gconv reads those int4 codes on the matrix pipe and leaves int4
    # codes, which the 1x1 conv behind it reads as they are -- no float32 tensor on either side of the gconv
    assert log == ["pack", "gconv_i4_mfma"], log
    assert conv_stores and conv_stores[-1] == _abi.STORE_I4 and _abi.STORE_F32 not in conv_stores[1:], conv_stores
    monkeypatch.undo()
    assert isinstance(nets.Model(None, spec).engine, engine.GraphModel)
    for cls in (engine.FusedModel, engine.ResidualFusedModel):
        with pytest.raises(_abi.NotFusable):
            cls(spec)
    with pytest.raises(_abi.NotFusable, match="gconv"):
        engine.FusedModel(resnext_spec(skip=False))
    with pytest.raises(_abi.NotFusable, match="gconv"):
        engine.ResidualFusedModel(resnext_spec(skip=False))


def concat_spec(seed=0):
    """The ShuffleNet / ResNeXt join: act (the skip) -> 3x3 gconv g = 4 -> BN -> act, concatenated with the skip, -> 1x1 conv."""
    rs = np.random.RandomState(290 + seed)
    k = lambda *shape: (rs.randint(-64, 65, shape) / 64.0).astype(np.float32)          # noqa: E731
    b = lambda n: (rs.randint(-8, 9, n) / 16.0).astype(np.float32)                     # noqa: E731
    act = lambda **kw: dict({"op": "act", "fn": "quantized_tanh", "nb": 4}, **kw)        # noqa: E731
    return [act(dst="skip"),
            {"op": "gconv", "kind": "quantized", "nb": 4, "kernel": k(3, 3, 4, 16), "bias": b(16), "groups": 4,
             "strides": (1, 1), "padding": "same", "dilation": (1, 1), "H": 1.0, "klm": np.float32(1.0)},
            {"op": "bn", "eps": 0.0, "gamma": (2.0 ** rs.randint(-3, 0, 16)).astype(np.float32) * rs.choice([-1, 1], 16).astype(np.float32),
             "beta": b(16), "mean": np.zeros(16, np.float32), "var": np.ones(16, np.float32)},
            act(dst="branch"), {"op": "concat", "srcs": ["branch", "skip"]},
            {"op": "conv", "kind": "quantized", "nb": 4, "kernel": k(1, 1, 32, 16), "bias": b(16), "strides": (1, 1),
             "padding": "same"}]


def test_gconv_codes_meet_a_skip_as_codes_in_a_concat(monkeypatch):
    from qnn_amd import engine
    spec = concat_spec()
    x = _features(2)
    f = np.float32
    gc, bn, conv = spec[1], spec[2], spec[5]
    skip = G.qact_code(G.FN_QUANTIZED_TANH, x, 8).astype(np.int64)
    case = dict(store=G.I4, groups=4, stride=1, same=True, dil=(1, 1), wkind=G.W_QUANT, wbits=4, x_bits=4,
                fn=G.FN_QUANTIZED_TANH, act_bits=4, out_store=G.I4)
    branch = G.reference(case, skip, gc["kernel"], gc["bias"], (bn["gamma"], bn["beta"]))
    cat = np.concatenate([branch, skip], -1)
    acc = np.einsum("nhwc,cf->nhwf", cat, G.quantize_weights(conv["kernel"], G.W_QUANT, 4)[1][0, 0])
    want = ((acc.astype(f) * f(2.0 ** -6)).astype(f) + conv["bias"]).astype(f)
    gm = engine.GraphModel(spec)
    gm.kernel_log = []
    conv_stores = _record_conv_stores(monkeypatch)
    y = host(gm(torch.from_numpy(x).cuda()))
    monkeypatch.undo()
    np.testing.assert_array_equal(y.view(np.uint32), want.view(np.uint32))
    log = gm.kernel_log
    # the gconv's codes are joined with the packed skip as codes and the 1x1 conv reads the joined codes
    assert "gconv_i4_mfma" in log and "concat_i4" in log and log.index("concat_i4") > log.index("gconv_i4_mfma"), log
    assert "unpack" not in log and "concat_f32" not in log, log
    assert conv_stores == [_abi.STORE_I4], conv_stores


def test_chain_on_layermodel_equals_graphmodel():
    from qnn_amd import engine
    spec = resnext_spec(skip=False)
    x = _features(1)
    want = resnext_reference(spec, x)
    xd = torch.from_numpy(x).cuda()
    np.testing.assert_array_equal(host(engine.LayerModel(spec)(xd)).view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(host(engine.GraphModel(spec)(xd)).view(np.uint32), want.view(np.uint32))


def test_float_gconv_behind_a_leaky_relu():
    from qnn_amd import engine
    rs = np.random.RandomState(70)
    k = (rs.randint(-64, 65, (3, 3, 2, 6)) / 64.0).astype(np.float32)
    b = (rs.randint(-8, 9, 6) / 16.0).astype(np.float32)
    gc = {"op": "gconv", "kind": "float", "kernel": k, "bias": b, "groups": 3, "strides": (2, 2), "padding": "valid",
          "dilation": (1, 1), "H": 1.0}
    x = (rs.randint(-64, 65, (2, 5, 4, 6)) / 64.0).astype(np.float32)
    leaky = np.where(x >= 0, x, (x * np.float32(0.3)).astype(np.float32)).astype(np.float32)
    c = dict(store=G.F32, groups=3, stride=2, same=False, dil=(1, 1), wkind=G.W_FLOAT, fn=G.FN_NONE, out_store=G.F32)
    want = G.reference(c, leaky, k, b, None)
    spec = [{"op": "act", "fn": "leaky_relu"}, gc]
    for cls in (engine.GraphModel, engine.LayerModel):
        np.testing.assert_array_equal(host(cls(spec)(torch.from_numpy(x).cuda())).view(np.uint32), want.view(np.uint32))
