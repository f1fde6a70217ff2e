"""quantized_relu / quantized_leakyrelu as fused conv epilogues on exact ties, tie neighbours, zeros and clip edges,
kernel by kernel.

The cases (qact_grid_cases.py; test_qact_grid_cpu.py proves what each carries) are the layers of the epilogue grid with
the two functions as the activation.  The un-folded int4 strip kernels restate both contracts in code units
(strip_qact<FN>, csrc/qnn_mfma_strip.hip) and are right only through one float32 rounding each -- fadd_rn(v, 1) and
fmul_rn(0.1f, v) --, which generic inputs never probe.  Every strip case runs twice, as routed and on k_conv_generic under
QNN_EPI_NO_STRIP: the raw words of the two runs are equal and each equals the numpy chain (the oracle's conv, bias, BN and
merge, then qrelu_cases.ACT[fn]) bit for bit; float32 outputs are compared by bit pattern, the sign of a zero included.

AN EPILOGUE CHANGE MUST KEEP THIS FILE GREEN (as test_gpu_epilogue_grid.py)."""
import numpy as np
import pytest

from qnn_amd import _abi, engine
import epilogue_grid_cases as G
import qact_grid_cases as A
import qrelu_cases as Q
import test_gpu_epilogue_grid as E

pytestmark = pytest.mark.gpu
FN = {A.RELU: _abi.FN_QUANTIZED_RELU, A.LEAKY: _abi.FN_QUANTIZED_LEAKYRELU}
CASES = A.cases()
_f32_layers = {}


def _layer(c):
    """(base tensors, prepacked weights, input as the store wants it, x_bits)."""
    if c["x_store"] != G.STORE_F32:
        b, (w, xp) = E._layer(c)
        return b, w, xp, b["x_bits"]
    b = G.base(*c["base"])
    if b["key"] not in _f32_layers:
        _f32_layers[b["key"]] = (engine._prepack(b["op"], _abi.STORE_F32, E.CUDA, stride=1, same_pad=True), E.dev(b["x"]))
    return (b,) + _f32_layers[b["key"]] + (0,)


def _run(c, a, pref, flags, w, xin, xbits, inv, shift, rkw):
    """One qnn_conv2d_forward: (kernel name, raw output words / floats, float32 values in the oracle's shape)."""
    _, N, H, W, cin, cout = c["base"][:6]
    with E._select(pref, flags):
        y, Ho, Wo = _abi.conv2d(w, xin, c["x_store"], xbits, N, H, W, inv, shift, FN[a["fn"]], a["nb"], c["pool"], a["store"],
                                **rkw)
        kern = _abi.last_kernel()
    raw = E.host(y)
    if a["store"] == _abi.STORE_F32:
        return kern, raw, raw
    return kern, raw, E.host(_abi.unpack(y, N * Ho * Wo, cout, a["store"], a["nb"])).reshape(N, Ho, Wo, cout)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_qact_epilogue_on_the_grid(c):
    b, w, xin, xbits = _layer(c)
    _, inv, shift = E._bn(c)
    rkw = E._res_kw(c)
    p = G.preactivation(c)
    strip = c["kernel"].startswith("strip_")
    ran, points, pinned = [], 0, set()
    for a in c["acts"]:
        want = G.expected(c, a, p)
        # as routed, then the twin: k_conv_generic under QNN_EPI_NO_STRIP (a strip case) or under IMPL_VALU
        kern, raw, got = _run(c, a, _abi.IMPL_AUTO, 0, w, xin, xbits, inv, shift, rkw)
        kt, rawt, gott = _run(c, a, _abi.IMPL_AUTO if strip else _abi.IMPL_VALU, _abi.EPI_NO_STRIP if strip else 0, w, xin, xbits,
                              inv, shift, rkw)
        ran.append("%s:%s/%s" % (a["id"], kern, kt))
        assert kern == c["kernel"] and kt == "generic", (c["id"], a["id"], kern, kt)
        if strip:
            assert kern.startswith("strip_i4_c%d" % c["base"][4]) and not kern.endswith("_lds"), kern
        for who, g_ in ((kern, got), (kt + " (twin)", gott)):
            assert g_.shape == want.shape, (c["id"], a["id"], who, g_.shape, want.shape)
            bad = np.count_nonzero(g_ != want)
            assert bad == 0, "%s %s: %s differs from the numpy chain in %d of %d outputs" % (c["id"], a["id"], who, bad, want.size)
            if a["store"] == _abi.STORE_F32:
                assert Q.same_bits(g_, want), (c["id"], a["id"], who)          # the sign of a zero is part of the contract
        assert np.array_equal(raw.view(np.int32), rawt.view(np.int32)), (c["id"], a["id"], kern, kt)
        points += want.size
        if strip and a["fn"] not in pinned:         # the dispatch, once per function: k_conv_ps has no capability for them
            pinned.add(a["fn"])
            kv, rawv, _ = _run(c, a, _abi.IMPL_VALU, 0, w, xin, xbits, inv, shift, rkw)
            assert kv == "generic" and np.array_equal(rawv, raw), (c["id"], a["id"], kv)
    print("[qact grid] %s: %s; %d points compared" % (c["id"], "; ".join(ran), points))


def test_no_fold_is_offered_for_the_two_functions():
    """A layer qnn_fold_prepare folds for quantized_tanh: None for quantized_relu and quantized_leakyrelu."""
    c = next(c for c in CASES if c["kernel"] == "strip_i4_c16" and c["epi"] == "dyadic")
    _, w, _, _ = _layer(c)
    _, inv, shift = E._bn(c)
    assert _abi.Fold.try_prepare(w, _abi.STORE_I4, 4, inv, shift, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4) is not None
    for fn in Q.FNS:
        assert _abi.Fold.try_prepare(w, _abi.STORE_I4, 4, inv, shift, FN[fn], 4, _abi.STORE_I4) is None, fn


PROJ = A.proj_cases()


@pytest.mark.parametrize("pc", PROJ, ids=[pc["id"] for pc in PROJ])
def test_in_launch_projection_on_the_grid(pc):
    """proj=: the shortcut is computed inside the strip launch.  Twin: the projection as a float32 tensor from a launch of
    its own, then the same layer on k_conv_generic with res_store = F32."""
    c = pc["main"]
    _, w, xp, _ = _layer(c)
    _, inv, shift = E._bn(c)
    _, N, H, W, cin, cout = c["base"][:6]
    pb = G.base(*pc["pbase"])
    _, _, Hb, Wb, pcin = pc["pbase"][:5]
    pw = engine._prepack(pb["op"], _abi.STORE_I4, E.CUDA, stride=2, same_pad=True)
    xbp = _abi.pack(E.dev(pb["x"]), pcin, _abi.FN_GRID, 4, _abi.STORE_I4)
    r32, _, _ = _abi.conv2d(pw, xbp, _abi.STORE_I4, 4, N, Hb, Wb)
    assert Q.same_bits(E.host(r32), pb["conv"])
    p = A.proj_preactivation(pc)
    ran = []
    for a in pc["acts"]:
        want = Q.ACT[a["fn"]](p, a["nb"])
        outs = []
        for flags, rkw in ((0, dict(post_scale=0.5, proj=(pw, xbp, Hb, Wb, 4))),
                           (_abi.EPI_NO_STRIP, dict(res=r32, res_store=_abi.STORE_F32, res_bits=0, post_scale=0.5))):
            with E._select(_abi.IMPL_AUTO, flags):
                y, Ho, Wo = _abi.conv2d(w, xp, _abi.STORE_I4, 4, N, H, W, inv, shift, FN[a["fn"]], a["nb"], 1, _abi.STORE_I4, **rkw)
                outs.append((_abi.last_kernel(), E.host(y)))
            got = E.host(_abi.unpack(y, N * Ho * Wo, cout, _abi.STORE_I4, a["nb"])).reshape(want.shape)
            bad = np.count_nonzero(got != want)
            assert bad == 0, "%s %s: %s differs from the numpy chain in %d of %d outputs" % (pc["id"], a["id"], outs[-1][0], bad, want.size)
        (kern, raw), (kt, rawt) = outs
        assert kern.startswith("strip_i4_c%d" % cin) and not kern.endswith("_lds") and kt == "generic", (kern, kt)
        assert np.array_equal(raw, rawt), (pc["id"], a["id"])
        ran.append("%s:%s/%s" % (a["id"], kern, kt))
    print("[qact grid] %s: %s; %d points compared" % (pc["id"], "; ".join(ran), p.size * len(pc["acts"])))


@pytest.mark.parametrize("dc", A.DENSE, ids=[dc["id"] for dc in A.DENSE])
def test_dense_epilogue_on_the_grid(dc):
    """qnn_dense_forward with the function as fn: the case's kernel against the numpy chain, by bit pattern, and (packed
    input) against k_dense_f32in on the same layer."""
    x, op, inv, shift, p = A.dense_layer(dc)
    n = x.shape[0]
    dinv, dshift = E.dev(inv), E.dev(shift)
    wf = engine._prepack(op, _abi.STORE_F32, E.CUDA)
    if dc["x_store"] == _abi.STORE_I4:
        wd, xin, bits = engine._prepack(op, _abi.STORE_I4, E.CUDA), _abi.pack(E.dev(x), dc["K"], _abi.FN_GRID, 4, _abi.STORE_I4), 4
    else:
        wd, xin, bits = wf, E.dev(x), 0
    ran = []
    for fn in Q.FNS:
        want = Q.ACT[fn](p, 4)
        got = E.host(_abi.dense(wd, xin, dc["x_store"], bits, n, dinv, dshift, FN[fn], 4))
        kern = _abi.last_kernel()
        assert kern == dc["kernel"], (dc["id"], kern)
        assert Q.same_bits(got, want), (dc["id"], fn, np.count_nonzero(got != want))
        twin = E.host(_abi.dense(wf, E.dev(x), _abi.STORE_F32, 0, n, dinv, dshift, FN[fn], 4))
        assert _abi.last_kernel() == "dense_f32" and Q.same_bits(twin, got), (dc["id"], fn)
        ran.append("%s:%s/dense_f32" % (fn, kern))
    print("[qact grid] %s (%s form): %s; %d points compared" % (dc["id"], dc["form"], "; ".join(ran), 2 * p.size))
