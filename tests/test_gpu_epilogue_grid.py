"""Every conv epilogue on exact rounding ties, exact zeros and clip edges, kernel by kernel.

The cases (epilogue_grid_cases.py; their content is proven by test_epilogue_grid_cpu.py) put the pre-activations of a layer
on the points where an epilogue can be subtly wrong and random BN constants never land: half-integers of quantized_tanh,
the threshold of binary_tanh, the clip edges.  Each case names the kernel it is for; the call is made with the QNN_EPI_*
flag that selects it, qnn_last_kernel is asserted, and the output is compared bit for bit with the oracle and with the same
call under IMPL_VALU (k_conv_ps / xnor / k_conv_generic: independent kernels; a dilated case -- strip_i4_c<cin>_dil, with its own copy of
the chain epilogue -- has k_conv_generic as its twin).  Every int4 -> int4 Q(4) call is repeated
with the folded epilogue: whatever qnn_fold_prepare decided, the bits are the same, and every channel it did fold is swept
over its whole accumulator domain (x 16 shortcut codes) against the oracle's chain.

AN EPILOGUE CHANGE MUST KEEP THIS FILE GREEN."""
import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine
from oracle import qnn_oracle as O
import epilogue_grid_cases as G
from test_gpu_fold import _chain_codes

pytestmark = pytest.mark.gpu
F32 = np.float32
CUDA = torch.device("cuda")
FN = {G.QT: _abi.FN_QUANTIZED_TANH, G.BT: _abi.FN_BINARY_TANH}
CASES = G.cases()
MATRIX_PIPE = ("strip_", "mfma_")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


_layers, _bns, _sweeps = {}, {}, {}


def _layer(c):
    """Prepacked weights and packed input of a case's base tensors: built once per (store, geometry)."""
    b = G.base(*c["base"])
    if b["key"] not in _layers:
        store, cin = c["x_store"], c["base"][4]
        w = engine._prepack(b["op"], store, CUDA, stride=b["op"]["strides"][0], same_pad=True)
        fn = _abi.FN_BINARY_TANH if store == _abi.STORE_BIN else _abi.FN_GRID
        _layers[b["key"]] = (w, _abi.pack(dev(b["x"]), cin, fn, b["x_bits"], store))
    return b, _layers[b["key"]]


def _bn(c):
    """(bn dict, inv, shift on the device) of a case, (None, None, None) without BN."""
    if c["sign"] is None:
        return None, None, None
    key = (c["base"][5], c["sign"])
    if key not in _bns:
        bn = G.dyadic_bn(*key)
        inv, shift = engine.bn_constants(bn)
        want = O.bn_constants(bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"])
        assert np.array_equal(inv, want[0]) and np.array_equal(shift, want[1])
        _bns[key] = (bn, dev(inv), dev(shift))
    return _bns[key]


def _res_kw(c):
    r = G.shortcut(c)
    if r is None:
        return {}
    cout = c["base"][5]
    if c["res"] == G.STORE_F32:
        return dict(res=dev(r), res_store=_abi.STORE_F32, res_bits=0, post_scale=c["post_scale"])
    return dict(res=_abi.pack(dev(r), cout, _abi.FN_GRID, c["res_bits"], c["res"]), res_store=c["res"],
                res_bits=c["res_bits"], post_scale=c["post_scale"])


class _select:
    """Implementation preference and QNN_EPI_* flags for the calls inside; both restored on the way out."""

    def __init__(self, pref, flags):
        self.pref, self.flags = pref, flags

    def __enter__(self):
        self.saved = _abi._default_flags
        _abi._default_flags = self.flags
        _abi.set_conv_impl(self.pref)

    def __exit__(self, *a):
        _abi._default_flags = self.saved
        _abi.set_conv_impl(_abi.IMPL_AUTO)


def _run(c, a, pref, w, xp, inv, shift, rkw, fold=None):
    """One qnn_conv2d_forward: (kernel name, raw output words / floats, float32 values in the oracle's shape)."""
    _, N, H, W, cin, cout = c["base"][:6]
    nb = a["nb"] if a["fn"] == G.QT else 0
    with _select(pref, c["flags"]):
        y, Ho, Wo = _abi.conv2d(w, xp, c["x_store"], G.base(*c["base"])["x_bits"], N, H, W, inv, shift, FN[a["fn"]], nb,
                                c["pool"], a["store"], fold=fold, **rkw)
        kern = _abi.last_kernel()
    raw = host(y)
    if a["store"] == _abi.STORE_F32:
        return kern, raw, raw
    return kern, raw, host(_abi.unpack(y, N * Ho * Wo, cout, a["store"], nb or 1)).reshape(N, Ho, Wo, cout)


def _sweep_fold(c, f, b, bn):
    """Every folded channel of `f` over its whole accumulator domain (x 16 shortcut codes): qnn_fold_eval == the oracle's
    chain.  Once per (layer, BN, shortcut form): the fold depends on nothing else.  Returns the points compared."""
    key = (c["base"], c["sign"], c["res"] is not None)
    if key in _sweeps:
        return _sweeps[key]
    op, cout = b["op"], c["base"][5]
    wc, wshift = O.weight_codes(op)
    assert wshift == 3
    wc = wc.reshape(-1, cout)
    hi, lo = np.maximum(wc * -8, wc * 7).sum(axis=0), np.minimum(wc * -8, wc * 7).sum(axis=0)
    A, _ = (host(t) for t in f.constants("cuda"))
    folded = np.nonzero(A != 0)[0]
    assert folded.size == f.folded
    points = 0
    for ch in folded:
        acc = np.arange(lo[ch], hi[ch] + 1, dtype=np.int32)
        dacc = dev(acc)
        for sc in (range(-8, 8) if c["res"] is not None else (None,)):
            scv = None if sc is None else np.full_like(acc, sc)
            got = host(f.eval(int(ch), dacc, None if scv is None else dev(scv)))
            np.testing.assert_array_equal(got, _chain_codes(acc, scv, ch, op, bn), err_msg="%s: channel %d shortcut %r"
                                          % (c["id"], ch, sc))
            points += acc.size
    _sweeps[key] = points
    return points


@pytest.mark.parametrize("c", [c for c in CASES if not c["head"]], ids=[c["id"] for c in CASES if not c["head"]])
def test_epilogue_on_the_grid(c):
    b, (w, xp) = _layer(c)
    bn, inv, shift = _bn(c)
    rkw = _res_kw(c)
    p = G.preactivation(c)
    ran = []
    for a in c["acts"]:
        want = G.expected(c, a, p)
        kern, raw, got = _run(c, a, _abi.IMPL_AUTO, w, xp, inv, shift, rkw)
        kv, rawv, gotv = _run(c, a, _abi.IMPL_VALU, w, xp, inv, shift, rkw)
        ran.append("%s:%s/%s" % (a["id"], kern, kv))
        if a["named"]:
            assert kern == c["kernel"], (c["id"], a["id"], kern)
            assert kv == c["valu"], (c["id"], a["id"], kv)
        assert not kv.startswith(MATRIX_PIPE), (c["id"], a["id"], kv)
        for who, k_, r_, g_ in (("auto", kern, raw, got), ("valu", kv, rawv, gotv)):
            assert g_.shape == want.shape, (c["id"], a["id"], who, g_.shape, want.shape)
            bad = np.count_nonzero(g_ != want)
            assert bad == 0, "%s %s: %s (%s) differs from the oracle in %d of %d outputs" % (c["id"], a["id"], k_, who, bad, want.size)
        assert np.array_equal(raw, rawv), (c["id"], a["id"], kern, kv)
        # the folded epilogue of the int4 -> int4 Q(4) calls
        if c["x_store"] == _abi.STORE_I4 and (a["fn"], a["nb"], a["store"]) == (G.QT, 4, _abi.STORE_I4):
            if c["d"] != 1:     # a dilated handle: qnn_fold_prepare refuses it with a reason, whatever the epilogue
                assert c["kernel"].endswith("_dil") and w.dilation == (c["d"], c["d"]), c["id"]
                with pytest.raises(_abi.QnnUnsupported, match="dilated"):
                    _abi.Fold(w, _abi.STORE_I4, 4, inv, shift, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4, **rkw)
                f = None
            else:
                f = _abi.Fold.try_prepare(w, _abi.STORE_I4, 4, inv, shift, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4, **rkw)
            if f is None:       # a shortcut form qnn_fold_prepare does not take (float32, 2 bit, post_scale other than 0.5),
                #                 a layer without a matrix-pipe weight image, or a dilated one (refused above)
                assert c["kernel"] == "generic" or c["d"] != 1 or (
                    c["res"] is not None and (c["res"], c["res_bits"], c["post_scale"]) != (_abi.STORE_I4, 4, 0.5)), c["id"]
                ran.append("fold: not offered")
                continue
            kf, rawf, gotf = _run(c, a, _abi.IMPL_AUTO, w, xp, inv, shift, rkw, fold=f)
            assert np.array_equal(rawf, raw), (c["id"], kf, np.count_nonzero(gotf != got))
            assert np.array_equal(gotf, want), (c["id"], kf)
            assert kf == c["kernel"] or kf == c["kernel"] + "_lds", (c["id"], kf)
            points = _sweep_fold(c, f, b, bn)
            ran.append("fold: %d / %d channels, usable %d, mode %d, kernel %s, %d points swept"
                       % (f.folded, f.channels, f.usable, f.mode, kf, points))
    print("[epilogue grid] %s: %s" % (c["id"], "; ".join(ran)))


@pytest.mark.parametrize("c", [c for c in CASES if c["head"]], ids=[c["id"] for c in CASES if c["head"]])
def test_conv_and_classifier_in_one_launch(c):
    """qnn_conv2d_dense_forward on the grid: the conv group's codes never leave the chip, so its epilogue is visible only
    through the logits -- equal to the two-launch form and to the oracle, with and without the fold."""
    b, (w, xp) = _layer(c)
    bn, inv, shift = _bn(c)
    N, H, W = c["base"][1:4]
    a = c["acts"][0]
    dense = G.head_dense()
    wd = engine._prepack(dense, _abi.STORE_I4, CUDA)
    pooled = G.expected(c, a)
    want = O.quantized_dense_call(pooled.reshape(N, -1), dense["kernel"], dense["bias"], nb=4)
    f = _abi.Fold.try_prepare(w, _abi.STORE_I4, 4, inv, shift, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4)
    assert f is not None
    for fold in (None, f):
        with _select(_abi.IMPL_AUTO, c["flags"]):
            y = _abi.conv2d_dense(w, wd, xp, _abi.STORE_I4, 4, N, H, W, inv, shift, _abi.FN_QUANTIZED_TANH, 4, None, None, fold=fold)
            assert y is not None and _abi.last_kernel() == c["kernel"] + "+dense", _abi.last_kernel()
            got = host(y)
            codes, _, _ = _abi.conv2d(w, xp, _abi.STORE_I4, 4, N, H, W, inv, shift, _abi.FN_QUANTIZED_TANH, 4, 2, _abi.STORE_I4,
                                      fold=fold)
            assert _abi.last_kernel() == c["kernel"], _abi.last_kernel()
            two = host(_abi.dense(wd, codes, _abi.STORE_I4, 4, N))
        np.testing.assert_array_equal(host(_abi.unpack(codes, N * 16, 64, _abi.STORE_I4, 4)).reshape(pooled.shape), pooled)
        np.testing.assert_array_equal(got, two)
        np.testing.assert_array_equal(got, want)
    print("[epilogue grid] %s: fold %d / %d channels, usable %d, %d points swept"
          % (c["id"], f.folded, f.channels, f.usable, _sweep_fold(c, f, b, bn)))
