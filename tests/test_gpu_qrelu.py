"""quantized_relu / quantized_leakyrelu on the GPU, bit for bit: the elementwise op and qnn_pack_f32 on the reference's
vectors, k_conv_generic over every input store, the un-folded int4 strip kernels (and the same calls on k_conv_generic
under QNN_EPI_NO_STRIP), and two small networks through every executor.  The numpy side is qrelu_cases.py, which
test_qrelu_cpu.py holds against golden/ref_qrelu.npz."""
import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine, nets
from oracle import qnn_oracle as O
import qrelu_cases as Q

pytestmark = pytest.mark.gpu
F32 = np.float32
CUDA = torch.device("cuda")
FN = {"quantized_relu": _abi.FN_QUANTIZED_RELU, "quantized_leakyrelu": _abi.FN_QUANTIZED_LEAKYRELU}
OP = {"quantized_relu": engine.quantized_ops.quantized_relu, "quantized_leakyrelu": engine.quantized_ops.quantized_leakyrelu}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


class _flags:
    """QNN_EPI_* flags for the calls inside; restored on the way out."""

    def __init__(self, flags):
        self.flags = flags

    def __enter__(self):
        self.saved = _abi._default_flags
        _abi._default_flags = self.flags

    def __exit__(self, *a):
        _abi._default_flags = self.saved


def _values(y, n, cout, store, nb, shape):
    return y if store == _abi.STORE_F32 else host(_abi.unpack(dev(y), n, cout, store, nb)).reshape(shape)


# ---- elementwise op and pack-on-load ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", Q.NBS)
@pytest.mark.parametrize("fn", Q.FNS)
def test_elementwise_and_pack_on_the_reference_vectors(fn, nb):
    x, relu, leaky = Q.fixture(nb)
    want = relu if fn == "quantized_relu" else leaky
    got = host(OP[fn](dev(x), nb))
    assert Q.same_bits(got, want), np.count_nonzero(got != want)
    odd = host(OP[fn](dev(x[:1003]), nb))                         # a length that is no multiple of four
    assert Q.same_bits(odd, want[:1003])
    for store in (_abi.STORE_I4, _abi.STORE_I8):
        if nb > store:
            continue
        for ch in (8, 5):                                          # whole words, and a ragged last word per pixel
            n = x.size // ch
            p = _abi.pack(dev(x[:n * ch].reshape(n, ch)), ch, FN[fn], nb, store)
            back = host(_abi.unpack(p, n, ch, store, nb)).reshape(-1)
            assert np.array_equal(back, want[:n * ch]), (fn, nb, store, ch)


# ---- k_conv_generic, every input store ----------------------------------------------------------------------------
GEN = dict(N=2, H=5, W=7, cin=5, cout=10)
IN_STORES = {"f32": (_abi.STORE_F32, "quantized", 4, 4), "bin": (_abi.STORE_BIN, "binary", 1, 1),
             "t2": (_abi.STORE_T2, "binary", 1, 0), "i4": (_abi.STORE_I4, "quantized", 4, 4),
             "i8": (_abi.STORE_I8, "quantized", 8, 8)}     # store, weight kind, weight bits, grid of the input values
_gen = {}


def _generic_layer(name):
    """Weights, input (packed as the store wants it), BN and residual of the 2x5x7, 5 -> 10 layer: once per store."""
    if name not in _gen:
        store, kind, wb, grid = IN_STORES[name]
        g = GEN
        op = Q.conv_op(kind, wb, 3, g["cin"], g["cout"], 1, seed=11)
        x = Q.grid_values((g["N"], g["H"], g["W"], g["cin"]), grid, seed=12)
        v0, _ = Q.conv_chain(x, op, None, "quantized_tanh", 4)
        bn = Q.bn_scaled(Q.bn_for(g["cout"], seed=13), float(v0.var()))
        inv, shift = engine.bn_constants(bn)
        w = engine._prepack(op, store, CUDA, stride=1, same_pad=True)
        xbits = {"f32": 0, "bin": 1, "t2": 1}.get(name, grid)
        xin = dev(x) if store == _abi.STORE_F32 else _abi.pack(dev(x), g["cin"], _abi.FN_GRID, max(xbits, 1), store)
        res = Q.grid_values((g["N"], g["H"], g["W"], g["cout"]), 4, seed=14)
        _gen[name] = dict(op=op, x=x, bn=bn, inv=dev(inv), shift=dev(shift), w=w, xin=xin, xbits=xbits, store=store, res=res)
    return _gen[name]


@pytest.mark.parametrize("fn", Q.FNS)
@pytest.mark.parametrize("name", sorted(IN_STORES))
def test_generic_kernel_every_store(name, fn):
    L, g = _generic_layer(name), GEN
    ran = 0
    for out_store, nb in ((_abi.STORE_F32, 4), (_abi.STORE_I4, 4), (_abi.STORE_I4, 2), (_abi.STORE_I8, 8)):
        for pool, with_res in ((1, False), (2, False), (1, True)):
            rkw, res = {}, None
            if with_res:
                res = L["res"]
                if out_store == _abi.STORE_F32:
                    rkw = dict(res=dev(res), res_store=_abi.STORE_F32, res_bits=0, post_scale=0.5)
                else:
                    rkw = dict(res=_abi.pack(dev(res), g["cout"], _abi.FN_GRID, 4, out_store), res_store=out_store, res_bits=4,
                               post_scale=0.5)
            pre, want = Q.conv_chain(L["x"], L["op"], L["bn"], fn, nb, pool, res, 0.5)
            y, Ho, Wo = _abi.conv2d(L["w"], L["xin"], L["store"], L["xbits"], g["N"], g["H"], g["W"], L["inv"], L["shift"],
                                    FN[fn], nb, pool, out_store, **rkw)
            assert _abi.last_kernel() == "generic", (name, _abi.last_kernel())
            got = _values(host(y), g["N"] * Ho * Wo, g["cout"], out_store, nb, want.shape)
            assert got.shape == want.shape and np.array_equal(got, want), (name, fn, out_store, nb, pool, with_res,
                                                                             np.count_nonzero(got != want))
            assert pre.min() < -1.0 and pre.max() > 1.0          # both clips are reached
            ran += 1
    assert ran == 12


@pytest.mark.parametrize("fn", Q.FNS)
def test_fused_on_load_dense_and_refusals(fn):
    """qnn_conv2d_forward_f32in with the function as in_fn, qnn_dense_forward with it as fn, and what the library refuses."""
    g = GEN
    op = Q.conv_op("quantized", 4, 3, g["cin"], g["cout"], 1, seed=21)
    rng = np.random.default_rng(22)
    xf = rng.uniform(-1.5, 1.5, (g["N"], g["H"], g["W"], g["cin"])).astype(F32)
    w = engine._prepack(op, _abi.STORE_I4, CUDA, stride=1, same_pad=True)
    y, _, _ = _abi.conv2d_f32in(w, dev(xf), FN[fn], 4)
    want = O.quantized_conv2d_call(Q.ACT[fn](xf, 4), op["kernel"], op["bias"], 4, None, (1, 1), "same")
    assert np.array_equal(host(y), want)
    # dense: packed input and float32 input, the function in the epilogue
    dk = {"op": "dense", "kind": "quantized", "nb": 4, "kernel": rng.uniform(-1, 1, (64, 10)).astype(F32),
          "bias": (rng.standard_normal(10) * 0.05).astype(F32)}
    xd = Q.grid_values((6, 64), 4, seed=23)
    wantd = Q.ACT[fn](O.quantized_dense_call(xd, dk["kernel"], dk["bias"], 4) * F32(0.25), 4)
    inv, shift = dev(np.full(10, 0.25, F32)), dev(np.zeros(10, F32))
    wd = engine._prepack(dk, _abi.STORE_I4, CUDA)
    got = host(_abi.dense(wd, _abi.pack(dev(xd), 64, _abi.FN_GRID, 4, _abi.STORE_I4), _abi.STORE_I4, 4, 6, inv, shift, FN[fn], 4))
    assert _abi.last_kernel().startswith("dense_") and np.array_equal(got, wantd), _abi.last_kernel()
    wf = engine._prepack(dk, _abi.STORE_F32, CUDA)
    got = host(_abi.dense(wf, dev(xd), _abi.STORE_F32, 0, 6, inv, shift, FN[fn], 4))
    assert _abi.last_kernel() == "dense_f32" and np.array_equal(got, wantd), _abi.last_kernel()
    # refusals, each with a reason: BIN output, act_bits above the store, the U8 entry, the fold, conv + classifier
    xp = _abi.pack(dev(Q.grid_values((g["N"], g["H"], g["W"], g["cin"]), 4, 24)), g["cin"], _abi.FN_GRID, 4, _abi.STORE_I4)
    for kw in (dict(out_store=_abi.STORE_BIN, act_bits=4), dict(out_store=_abi.STORE_I4, act_bits=5)):
        with pytest.raises(_abi.QnnError, match="does not fit|BIN output"):
            _abi.conv2d(w, xp, _abi.STORE_I4, 4, g["N"], g["H"], g["W"], fn=FN[fn], **kw)
    w8 = engine._prepack(op, _abi.STORE_F32, CUDA, stride=1, same_pad=True)
    xu8 = dev(rng.integers(0, 256, (g["N"], g["H"], g["W"], g["cin"]), dtype=np.uint8))
    with pytest.raises(_abi.QnnError, match=r"\(-2\).*QNN_STORE_U8"):
        _abi.conv2d(w8, xu8, _abi.STORE_U8, 0, g["N"], g["H"], g["W"], fn=FN[fn], act_bits=4, out_store=_abi.STORE_I4)
    S = _strip_layer(STRIP[0])                                   # a layer qnn_fold_prepare folds for quantized_tanh
    assert _abi.Fold.try_prepare(S["w"], _abi.STORE_I4, 4, S["inv"], S["shift"], _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4) is not None
    assert _abi.Fold.try_prepare(S["w"], _abi.STORE_I4, 4, S["inv"], S["shift"], FN[fn], 4, _abi.STORE_I4) is None


# ---- the un-folded int4 strip family ----------------------------------------------------------------------------------
# (cin, cout, stride, shortcut, H, W, act bits): shortcut None | "i4" (packed codes) | "f32" | "proj" (in-launch projection)
STRIP = [(16, 16, 1, None, 7, 20, 4), (16, 16, 1, "i4", 7, 20, 4), (16, 16, 1, "f32", 7, 20, 4),
         (32, 32, 1, None, 7, 20, 4), (32, 32, 1, "i4", 7, 20, 4), (32, 32, 1, "f32", 7, 20, 4),
         (64, 64, 1, None, 7, 20, 4), (64, 64, 1, "i4", 7, 20, 4), (64, 64, 1, "f32", 7, 20, 4),
         (16, 32, 2, None, 7, 20, 4), (32, 64, 2, None, 7, 20, 4), (32, 32, 1, "proj", 7, 20, 4),
         (16, 16, 1, None, 1, 3, 2), (32, 32, 1, "i4", 1, 3, 3), (64, 64, 1, "f32", 1, 3, 4), (16, 32, 2, None, 1, 3, 4)]
_strip = {}


def _strip_layer(case):
    """Everything of a strip case that does not depend on the activation: once per case."""
    if case not in _strip:
        cin, cout, stride, short, H, W, nb = case
        N = 2
        bias = cin != 32                                          # both BIAS instantiations
        op = Q.conv_op("quantized", 4, 3, cin, cout, stride, seed=100 + cin + stride, bias=bias)
        x = Q.grid_values((N, H, W, cin), 4, seed=31 + cin)
        Ho, Wo = -(-H // stride), -(-W // stride)
        v0, _ = Q.conv_chain(x, op, None, "quantized_tanh", 4)
        bn = Q.bn_scaled(Q.bn_for(cout, seed=32 + cin, spread=2.0 if short else 1.0), float(v0.var()))
        inv, shift = engine.bn_constants(bn)
        L = dict(N=N, op=op, x=x, bn=bn, inv=dev(inv), shift=dev(shift), Ho=Ho, Wo=Wo,
                 w=engine._prepack(op, _abi.STORE_I4, CUDA, stride=stride, same_pad=True),
                 xp=_abi.pack(dev(x), cin, _abi.FN_GRID, 4, _abi.STORE_I4), res=None, rkw={}, rkw_two=None)
        if short == "i4":
            L["res"] = Q.grid_values((N, Ho, Wo, cout), 4, seed=33)
            L["rkw"] = dict(res=_abi.pack(dev(L["res"]), cout, _abi.FN_GRID, 4, _abi.STORE_I4), res_store=_abi.STORE_I4,
                            res_bits=4, post_scale=0.5)
        elif short == "f32":
            L["res"] = np.random.default_rng(34).uniform(-2, 2, (N, Ho, Wo, cout)).astype(F32)
            L["rkw"] = dict(res=dev(L["res"]), res_store=_abi.STORE_F32, res_bits=0, post_scale=0.5)
        elif short == "proj":
            pop = Q.conv_op("quantized", 4, 1, cin // 2, cout, 2, seed=35, bias=True)
            xb = Q.grid_values((N, 2 * H - 1, 2 * W, cin // 2), 4, seed=36)       # an odd and an even size: ceil(./2) = H, W
            L["res"] = O.quantized_conv2d_call(xb, pop["kernel"], pop["bias"], 4, None, (2, 2), "same")
            assert L["res"].shape == (N, H, W, cout)
            pw = engine._prepack(pop, _abi.STORE_I4, CUDA, stride=2, same_pad=True)
            xbp = _abi.pack(dev(xb), cin // 2, _abi.FN_GRID, 4, _abi.STORE_I4)
            L["rkw"] = dict(post_scale=0.5, proj=(pw, xbp, 2 * H - 1, 2 * W, 4))
            # the two-launch form k_conv_generic can run: the projection as a float32 tensor, then a float32 shortcut
            r32, _, _ = _abi.conv2d(pw, xbp, _abi.STORE_I4, 4, N, 2 * H - 1, 2 * W)
            assert np.array_equal(host(r32), L["res"])
            L["rkw_two"] = dict(res=r32, res_store=_abi.STORE_F32, res_bits=0, post_scale=0.5)
        _strip[case] = L
    return _strip[case]


@pytest.mark.parametrize("fn", Q.FNS)
@pytest.mark.parametrize("case", STRIP, ids=["c%d_%d_s%d_%s_%dx%d_q%d" % c for c in STRIP])
def test_strip_kernels(case, fn):
    cin, cout, stride, short, H, W, nb = case
    L = _strip_layer(case)
    pre, want = Q.conv_chain(L["x"], L["op"], L["bn"], fn, nb, 1, L["res"], 0.5)
    m = 2 ** (nb - 1)
    if H > 1:                                                      # both clips, zero and both BN signs are exercised
        assert pre.min() < -1.05 and pre.max() > 1.05 and (L["bn"]["gamma"] > 0).any() and (L["bn"]["gamma"] < 0).any()
        codes = set(np.unique(want * F32(m)).tolist())
        assert {0, m - 1} <= codes and (fn == "quantized_relu" or min(codes) < 0), codes

    def call(flags, rkw):
        with _flags(flags):
            y, Ho, Wo = _abi.conv2d(L["w"], L["xp"], _abi.STORE_I4, 4, L["N"], H, W, L["inv"], L["shift"], FN[fn], nb, 1,
                                    _abi.STORE_I4, **rkw)
            assert (Ho, Wo) == (L["Ho"], L["Wo"])
            return _abi.last_kernel(), host(y)

    kern, raw = call(0, L["rkw"])
    assert kern.startswith("strip_i4_c%d" % cin) and not kern.endswith("_lds"), kern
    kgen, rawg = call(_abi.EPI_NO_STRIP, L["rkw_two"] or L["rkw"])
    assert kgen == "generic", kgen
    assert np.array_equal(raw, rawg), (kern, np.count_nonzero(raw != rawg))
    got = _values(raw, L["N"] * L["Ho"] * L["Wo"], cout, _abi.STORE_I4, nb, want.shape)
    assert np.array_equal(got, want), (kern, np.count_nonzero(got != want))


def test_quantized_tanh_keeps_its_kernels():
    """The same strip call with quantized_tanh still takes the kernels it took (the LDS-staged form with a fold included)."""
    L = _strip_layer(STRIP[0])
    y, _, _ = _abi.conv2d(L["w"], L["xp"], _abi.STORE_I4, 4, L["N"], 7, 20, L["inv"], L["shift"], _abi.FN_QUANTIZED_TANH, 4, 1,
                          _abi.STORE_I4)
    assert _abi.last_kernel() == "strip_i4_c16"
    _, want = Q.conv_chain(L["x"], L["op"], L["bn"], "quantized_tanh", 4)
    assert np.array_equal(host(_abi.unpack(y, L["N"] * 7 * 20, 16, _abi.STORE_I4, 4)).reshape(want.shape), want)


# ---- whole networks ------------------------------------------------------------------------------------------------------
_nets = {}


def _net(arch, fn):
    if (arch, fn) not in _nets:
        if arch == "RESNET":
            # 16 x 16 images leave a 4 x 4 map in front of the classifier, smaller than AveragePooling2D(8) of
            # models/resnet.py:134: the pool of this small network covers the whole map (size 4), 64 features as ever
            cf = nets.Config(network_type="full-qnn", wbits=4, abits=4, architecture="RESNET", nres=1, dim=16)
            spec = nets.build_spec(nets.Config(network_type="full-qnn", wbits=4, abits=4, architecture="RESNET", nres=1, dim=32),
                                   5, quantized_activation=fn)
            for op in spec:
                if op["op"] == "avgpool":
                    op["size"] = 4
        else:
            cf = nets.Config(network_type="full-qnn", wbits=4, abits=4, architecture="VGG", dim=8, nfa=16, nfb=32, nfc=64)
            spec = nets.build_spec(cf, 5, quantized_activation=fn)
        x = nets.synthetic_images(cf, 3, 6)
        _nets[arch, fn] = (cf, spec, x, Q.run_spec(spec, x, float_conv="device"), nets.synthetic_images_u8(cf, 3, 6))
    return _nets[arch, fn]


@pytest.mark.parametrize("fn", Q.FNS)
@pytest.mark.parametrize("arch", ["RESNET", "VGG"])
def test_whole_networks_through_every_executor(arch, fn):
    cf, spec, x, want, xu8 = _net(arch, fn)
    xd = dev(x)
    assert want.shape == (3, 10) and np.isfinite(want).all()
    if arch == "RESNET":
        m = engine.ResidualFusedModel(spec)
        m.kernel_log = []
        got = host(m(xd))
        assert np.array_equal(got, want), np.abs(got - want).max()
        assert any(k.startswith("strip_i4_c16") for k in m.kernel_log) and any(k.startswith("strip_i4_c32") for k in m.kernel_log), m.kernel_log
        assert not m._folds or all(f is None for f in m._folds.values())          # no fold is asked for
        with pytest.raises(_abi.NotFusable):
            engine.FusedModel(spec)
    else:
        m = engine.FusedModel(spec)
        m.kernel_log = []
        got = host(m(xd))
        assert np.array_equal(got, want), np.abs(got - want).max()
        assert all(st.get(k) is None for st in m.steps for k in ("fold_img", "fold_i4"))                  # no fold is asked for
        assert np.array_equal(host(engine.ResidualFusedModel(spec)(xd)), want)
    for exact in ("exact", "auto"):
        e = type(m)(spec, first_layer=exact)
        assert np.array_equal(host(e(xd)), want), exact
    assert np.array_equal(host(engine.GraphModel(spec)(xd)), want)
    assert np.array_equal(host(engine.LayerModel(spec)(xd)), want)
    # uint8 images: the U8 entry is not defined for these functions, the first layer runs on bytes / 255 in float32
    want8 = Q.run_spec(spec, xu8.astype(F32) / F32(255), float_conv="device")
    assert np.array_equal(host(m(dev(xu8))), want8)
    # Model.predict: the pipelined engine, full batches replayed and a ragged tail
    model = nets.Model(cf, spec)
    assert np.array_equal(model.predict(x, batch_size=2), want)
    assert np.array_equal(host(model.predict(dev(xu8), batch_size=2)), want8)
