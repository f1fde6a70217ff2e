"""Packed codes plus a device-resident scale on the GPU (include/qnn_abi_scaled.h; csrc/qnn_maxact_pack.hip and the scaled
forms of k_conv_generic / k_dense_packed): the pack kernel against scaled_cases.codes, the scaled consumers on every route
that lists CAP_XSCALE against the integer reference and against the float32 entry, the refusals of the scaled entries, and
GraphModel with scaled_codes on and off.  test_scaled_cpu.py proves the references on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine, nets, shard
import maxrelu_cases as C
import scaled_cases as S

pytestmark = pytest.mark.gpu
F32 = np.float32
CUDA = torch.device("cuda")
FN = {"quantized_maxrelu": _abi.FN_QUANTIZED_MAXRELU, "quantized_leakymaxrelu": _abi.FN_QUANTIZED_LEAKYMAXRELU}
quantized_ops = engine.quantized_ops


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _apply(x, fn, nb, ws):
    y = torch.empty_like(x)
    _abi.check(_abi.load().qnn_maxact_apply_f32(_abi.ptr(x), _abi.ptr(y), x.numel(), FN[fn], nb, _abi.ptr(ws),
                                                _abi.stream_ptr()), "qnn_maxact_apply_f32")
    return y


def _word(M):
    """A workspace as pass 1 leaves it for maximum M."""
    return dev(np.array([np.asarray(M, F32).view(np.int32), 0, 0, 0], np.int32))


# ---- 1. the pack kernel ------------------------------------------------------------------------------------------------
# three binades of MAXIMA, an exact power of two of the ambiguous band, and the two ends of the exact range
PACK_MAXIMA = (C.MAXIMA[0], C.MAXIMA[4], C.MAXIMA[10], C.AMBIGUOUS[17], F32(2.0 ** -64), F32(2.0 ** 64))
STORES = ((_abi.STORE_I4, 2), (_abi.STORE_I4, 3), (_abi.STORE_I4, 4), (_abi.STORE_I8, 8), (_abi.STORE_I8, 4))


def _pack_input(M, pixels, ch, seed):
    x = C.uniform_inputs(M, seed, pixels * ch).reshape(pixels, ch)
    x.reshape(-1)[(pixels * ch) // 2] = M
    return x


@pytest.mark.parametrize("store,nb", STORES)
@pytest.mark.parametrize("fn", C.FNS)
def test_pack_kernel(fn, store, nb):
    assert float(C.AMBIGUOUS[17]) == 1.0
    seed = 0
    for ch in (8, 16, 64, 5, 12):                      # whole words (the 16-byte form); a ragged last word (the slow form)
        for pixels in (1, 7, 1027):
            for M in PACK_MAXIMA:
                seed += 1
                x = _pack_input(M, pixels, ch, seed)
                xd = dev(x)
                ws = quantized_ops.maxact_word(xd)
                assert host(ws).view(F32)[0] == M
                want = S.pack_words(S.codes(x, nb, fn, M), store)
                got = host(_abi.maxact_pack(xd, ch, FN[fn], nb, store, ws)).view(np.uint32)
                assert np.array_equal(got, want), (ch, pixels, float(M))
                assert not (got[:, -1] & np.uint32(S.spare_mask(ch, store))).any()
                # DUAL: the same codes, and the float32 tensor of the apply pass bit for bit
                y = torch.full_like(xd, 7.0)
                got = host(_abi.maxact_pack(xd, ch, FN[fn], nb, store, ws, y=y)).view(np.uint32)
                assert np.array_equal(got, want) and C.same_bits(host(y), host(_apply(xd, fn, nb, ws)))
                assert C.same_bits(host(y), C.maxact(x, nb, fn))
    assert _abi.last_kernel() == "maxact_pack_i%d_dual" % store


@pytest.mark.parametrize("fn", C.FNS)
def test_pack_in_place_unaligned_and_out_of_range(fn):
    nb, store = 4, _abi.STORE_I4
    for ch, pixels in ((16, 1027), (12, 257)):
        M = C.MAXIMA[5]
        x = _pack_input(M, pixels, ch, 99)
        want = S.pack_words(S.codes(x, nb, fn, M), store)
        # in place: y == x
        xd = dev(x)
        ws = quantized_ops.maxact_word(xd)
        got = host(_abi.maxact_pack(xd, ch, FN[fn], nb, store, ws, y=xd)).view(np.uint32)
        assert np.array_equal(got, want) and C.same_bits(host(xd), C.maxact(x, nb, fn))
        # a pointer that is not 16-byte aligned takes the one-word-per-lane form
        buf = dev(np.concatenate([[F32(0)], x.reshape(-1)]).astype(F32))
        xu = buf[1:].reshape(pixels, ch)
        assert xu.data_ptr() % 16 == 4 and xu.is_contiguous()
        y = torch.empty_like(buf)[1:].reshape(pixels, ch)
        got = host(_abi.maxact_pack(xu, ch, FN[fn], nb, store, ws, y=y)).view(np.uint32)
        assert np.array_equal(got, want) and C.same_bits(host(y), C.maxact(x, nb, fn))
        # M <= 0 and M > 2^64: codes all zero, y quiet NaN everywhere
        xd = dev(x)
        for ws in (_word(0.0), _word(2.0 ** 64 * 1.0001), quantized_ops.maxact_word(dev(-np.abs(x) - F32(0.5)))):
            for st, b in ((_abi.STORE_I4, 4), (_abi.STORE_I8, 8)):
                y = torch.zeros_like(xd)
                assert not host(_abi.maxact_pack(xd, ch, FN[fn], b, st, ws, y=y)).any()
                assert np.array_equal(host(y).view(np.uint32), np.full(x.shape, 0x7FC00000, np.uint32))
                assert not host(_abi.maxact_pack(xd, ch, FN[fn], b, st, ws)).any()


@pytest.mark.parametrize("fn", C.FNS)
def test_pack_valid_rows_keep_the_padding_out_of_the_maximum(fn):
    x = C.uniform_inputs(F32(1.0), 5, 6 * 5 * 8).reshape(6, 5, 8)
    x[1, 2, 3] = F32(1.3)
    x[4:] = F32(5.0)                                             # the padded rows carry a larger value: it must not win
    xd = dev(x)
    with shard.sharded(None, valid_rows=4):
        ws = quantized_ops.maxact_word(xd)
    got = host(_abi.maxact_pack(xd, 8, FN[fn], 4, _abi.STORE_I4, ws)).view(np.uint32)
    want = S.pack_words(S.codes(x, 4, fn, F32(1.3)).reshape(-1, 8), _abi.STORE_I4)
    assert np.array_equal(got, want)
    assert not np.array_equal(want, S.pack_words(S.codes(x, 4, fn, F32(5.0)).reshape(-1, 8), _abi.STORE_I4))


# ---- 2. the scaled consumers, one case per route that lists CAP_XSCALE -------------------------------------------------------
def _weights(op, store):
    if op["op"] == "dense":
        return engine._prepack(op, store, CUDA)
    return engine._prepack(op, store, CUDA, stride=op["strides"][0], same_pad=op["padding"] == "same")


def _device_epilogue(epi):
    kw = {}
    if "bn" in epi:
        kw["bn_inv"], kw["bn_shift"] = (dev(a) for a in engine.bn_constants(epi["bn"]))
    if "res" in epi:
        kw.update(res=dev(epi["res"]), res_store=_abi.STORE_F32, post_scale=epi["post_scale"])
    return kw


def _run(op, w, x, store, bits, shape, x_scale=None, trick=None, **kw):
    if op["op"] == "dense":
        return _abi.dense(w, x, store, bits, shape[0], kw.get("bn_inv"), kw.get("bn_shift"), x_scale=x_scale)
    N, H, W, _ = shape
    return _abi.conv2d(w, x, store, bits, N, H, W, trick=trick, x_scale=x_scale, **kw)[0]


@pytest.mark.parametrize("name", sorted(S.CONSUMERS))
def test_scaled_consumers(name):
    op, shape, nb, store, kernel, pieces = S.CONSUMERS[name]
    fn = "quantized_leakymaxrelu"
    w, wf = _weights(op, store), _weights(op, _abi.STORE_F32)
    for P in S.SCALES + (2.0 ** -64, 2.0 ** 64):
        x, M = S.consumer_input(name, P, fn)
        xd = dev(x)
        ws = quantized_ops.maxact_word(xd)
        y = torch.empty_like(xd)
        xp = _abi.maxact_pack(xd, shape[-1], FN[fn], nb, store, ws, y=y)
        k = S.codes(x, nb, fn, M)
        bare = S.scaled_reference(k, nb, M, op)
        for which in S.epilogue_sets(pieces) if P in S.SCALES else [()]:
            epi = S.epilogue_args(name, which, bare.shape, P)
            kw = _device_epilogue(epi)
            got = host(_run(op, w, xp, store, nb, shape, x_scale=ws, trick=epi.get("trick"), **kw))
            assert _abi.last_kernel() == kernel, (name, which)
            want = S.scaled_reference(k, nb, M, op, **epi)
            assert got.shape == want.shape and C.same_bits(got, want), (name, P, which)
            # and the float32 entry on the float32 activation of the same pass
            flt = host(_run(op, wf, y, _abi.STORE_F32, 0, shape, trick=epi.get("trick"), **kw))
            assert "scaled" not in _abi.last_kernel() and C.same_bits(got, flt), (name, P, which)
    # a word outside the exact range: NaN everywhere
    for bad in (_word(0.0), _word(np.inf), _word(2.0 ** 64 * 1.0001)):
        assert np.isnan(host(_run(op, w, xp, store, nb, shape, x_scale=bad))).all()


# ---- 3. refusals of the scaled entries ---------------------------------------------------------------------------------
def test_scaled_entries_refuse_by_name():
    import qrelu_cases as Q
    N, H, W, cin, cout = 2, 5, 7, 16, 16
    op = Q.conv_op("quantized", 4, 3, cin, cout, 1, seed=41)
    w = engine._prepack(op, _abi.STORE_I4, CUDA, stride=1, same_pad=True)
    xg = Q.grid_values((N, H, W, cin), 4, seed=42)
    xp = _abi.pack(dev(xg), cin, _abi.FN_GRID, 4, _abi.STORE_I4)
    ws = _word(1.0)
    named = "qnn_conv2d_forward_scaled"
    for out_store, fn in ((_abi.STORE_I4, _abi.FN_QUANTIZED_TANH), (_abi.STORE_I8, _abi.FN_QUANTIZED_TANH),
                          (_abi.STORE_BIN, _abi.FN_BINARY_TANH)):
        with pytest.raises(_abi.QnnUnsupported, match=named):
            _abi.conv2d(w, xp, _abi.STORE_I4, 4, N, H, W, fn=fn, act_bits=4, out_store=out_store, x_scale=ws)
    inv, shift = (dev(a) for a in engine.bn_constants(Q.bn_scaled(Q.bn_for(16, seed=46), 9 * 16 * 0.1)))
    fold = _abi.Fold.try_prepare(w, _abi.STORE_I4, 4, inv, shift, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4)
    assert fold is not None
    with pytest.raises(_abi.QnnUnsupported, match=named):
        _abi.conv2d(w, xp, _abi.STORE_I4, 4, N, H, W, inv, shift, fold=fold, x_scale=ws)
    pw = engine._prepack(Q.conv_op("quantized", 4, 1, 8, 16, 2, seed=47), _abi.STORE_I4, CUDA, stride=2, same_pad=True)
    px = _abi.pack(dev(Q.grid_values((N, 2 * H, 2 * W, 8), 4, seed=48)), 8, _abi.FN_GRID, 4, _abi.STORE_I4)
    with pytest.raises(_abi.QnnUnsupported, match=named):
        _abi.conv2d(w, xp, _abi.STORE_I4, 4, N, H, W, proj=(pw, px, 2 * H, 2 * W, 4), post_scale=0.5, x_scale=ws)
    with pytest.raises(_abi.QnnUnsupported, match=named):
        _abi.conv2d(w, xp, _abi.STORE_I4, 4, N, H, W, pool=2, x_scale=ws)
    for x_store in (_abi.STORE_BIN, _abi.STORE_T2, _abi.STORE_F32, _abi.STORE_U8):
        with pytest.raises(_abi.QnnUnsupported, match=named):
            _abi.conv2d(w, xp, x_store, 4, N, H, W, x_scale=ws)
    # a NULL word (the Python wrapper takes None for "no scale": the entry itself)
    epi = _abi.make_epilogue(None, None, _abi.FN_NONE, 0, 1, _abi.STORE_F32)
    y = torch.empty((N, H, W, cout), dtype=torch.float32, device=CUDA)
    lib = _abi.load()
    assert lib.qnn_conv2d_forward_scaled(w.handle, _abi.ptr(xp), _abi.STORE_I4, 4, N, H, W, ctypes.byref(epi), None, _abi.ptr(y),
                                         _abi.stream_ptr()) == -1
    assert named.encode() in lib.qnn_last_error()
    # the dense entry
    dk = {"op": "dense", "kind": "quantized", "nb": 4, "kernel": np.random.default_rng(43).uniform(-1, 1, (64, 10)).astype(F32),
          "bias": None}
    wd = engine._prepack(dk, _abi.STORE_I4, CUDA)
    xd = _abi.pack(dev(Q.grid_values((6, 64), 4, seed=44)), 64, _abi.FN_GRID, 4, _abi.STORE_I4)
    named = "qnn_dense_forward_scaled"
    with pytest.raises(_abi.QnnUnsupported, match=named):
        _abi.dense(wd, xd, _abi.STORE_I4, 4, 6, fn=_abi.FN_QUANTIZED_TANH, act_bits=4, out_store=_abi.STORE_I4, x_scale=ws)
    for x_store in (_abi.STORE_BIN, _abi.STORE_T2, _abi.STORE_F32):
        with pytest.raises(_abi.QnnUnsupported, match=named):
            _abi.dense(wd, xd, x_store, 4, 6, x_scale=ws)
    yd = torch.empty((6, 10), dtype=torch.float32, device=CUDA)
    assert lib.qnn_dense_forward_scaled(wd.handle, _abi.ptr(xd), _abi.STORE_I4, 4, 6, ctypes.byref(epi), None, _abi.ptr(yd),
                                        _abi.stream_ptr()) == -1
    assert named.encode() in lib.qnn_last_error()
    with pytest.raises(_abi.QnnError, match="prepacked as a 3x3 conv"):
        _abi.dense(w, xd, _abi.STORE_I4, 4, 6, x_scale=ws)
    # a layer beyond the 2^24 bound of the contract (8 / 8 bits, K = 1152)
    op8 = Q.conv_op("quantized", 8, 3, 128, 8, 1, seed=49)
    w8 = engine._prepack(op8, _abi.STORE_I8, CUDA, stride=1, same_pad=True)
    x8 = _abi.pack(dev(Q.grid_values((N, H, W, 128), 8, seed=50)), 128, _abi.FN_GRID, 8, _abi.STORE_I8)
    with pytest.raises(_abi.QnnUnsupported, match="qnn_conv2d_forward_scaled.*2\\^24"):
        _abi.conv2d(w8, x8, _abi.STORE_I8, 8, N, H, W, x_scale=ws)
    # the two functions stay refused as an epilogue, word for word
    for fn in _abi.MAXACT_FNS:
        with pytest.raises(_abi.QnnUnsupported, match="qnn_quantized_maxact_f32"):
            _abi.conv2d(w, xp, _abi.STORE_I4, 4, N, H, W, fn=fn, act_bits=4, x_scale=ws)
    # and an ordinary call of the same layer takes the kernel it took
    _abi.conv2d(w, xp, _abi.STORE_I4, 4, N, H, W, inv, shift, _abi.FN_QUANTIZED_TANH, 4, 1, _abi.STORE_I4)
    assert _abi.last_kernel() in ("strip_i4_c16", "strip_i4_c16_lds")
    _abi.conv2d(w, xp, _abi.STORE_I4, 4, N, H, W)
    assert "scaled" not in _abi.last_kernel()


# ---- 4. GraphModel -------------------------------------------------------------------------------------------------------
_nets = {}


def _net(arch, nt, fn):
    """The four small networks of test_gpu_maxrelu.py (rebuilt here), 3 images, and their numpy runs: the whole batch at
    once, and in batches of 2."""
    if (arch, nt, fn) not in _nets:
        kw = dict(network_type=nt, wbits=4, abits=4)
        if arch == "RESNET":
            cf = nets.Config(architecture="RESNET", nres=1, dim=16, **kw)
            spec = nets.build_spec(nets.Config(architecture="RESNET", nres=1, dim=32, **kw), 5, quantized_activation=fn, batch_scaled=True)
            for op in spec:
                if op["op"] == "avgpool":
                    op["size"] = 4
        else:
            cf = nets.Config(architecture="VGG", dim=8, nfa=16, nfb=32, nfc=64, **kw)
            spec = nets.build_spec(cf, 5, quantized_activation=fn, batch_scaled=True)
        x = nets.synthetic_images(cf, 3, 6)
        _nets[arch, nt, fn] = (cf, spec, x, C.run_spec(spec, x), C.run_spec(spec, x, batch_size=2))
    return _nets[arch, nt, fn]


@pytest.mark.parametrize("fn", C.FNS)
@pytest.mark.parametrize("nt", ["full-qnn", "qbnn"])
@pytest.mark.parametrize("arch", ["RESNET", "VGG"])
def test_graph_model_with_scaled_codes(arch, nt, fn):
    cf, spec, x, want, want2 = _net(arch, nt, fn)
    xd = dev(x)
    off, on = engine.GraphModel(spec, scaled_codes=False), engine.GraphModel(spec, scaled_codes=True)
    assert engine.GraphModel(spec).scaled_codes is False         # the default (profiles/scaled/README.md)
    off.kernel_log, on.kernel_log = [], []
    a, b = host(off(xd)), host(on(xd))
    assert C.same_bits(a, want) and C.same_bits(b, want)
    assert not any("scaled" in k or "maxact_pack" in k for k in off.kernel_log)
    # In these four networks no consumer takes the scaled route, and the planner must leave every one of them where it was:
    # the VGG's activations are read by max-pools (conv - BN - act - maxpool), which read float32, and the ResNet's by 16 / 32 /
    # 64-channel convolutions that the float32 route runs on the f32 matrix pipe (engine._scaled_route_pays: their scaled call
    # would fall to k_conv_generic) and by the average pool.  test_a_vgg_shaped_network_takes_the_matrix_pipe and the two
    # hand-written specs below are the networks whose layers do take it.
    assert on.kernel_log == off.kernel_log
    if arch == "RESNET":
        conv = next(op for op in spec if op["op"] == "conv" and op["kernel"].shape[2] == 16)
        assert not engine._scaled_route_pays(conv, _abi.STORE_I4)
    for cls in (engine.FusedModel, engine.ResidualFusedModel):
        with pytest.raises(_abi.NotFusable, match="maximum of the whole batch"):
            cls(spec)
    # Model.predict: full batches replayed from captured graphs and a ragged tail, twice to the same bits
    model = nets.Model(cf, spec, scaled_codes=True)
    assert isinstance(model.engine, engine.GraphModel) and model.engine.scaled_codes
    assert nets.Model(cf, spec).engine.scaled_codes is False
    first = model.predict(x, batch_size=2)
    assert C.same_bits(first, want2)
    assert np.array_equal(model.predict(x, batch_size=2), first)


def _conv(kind, nb, kh, cin, cout, seed, **kw):
    op = S._op(kind, nb, kh, cin, cout, 1, "same", seed)
    op.update(kw)
    return op


def _bn(cout, seed, var):
    import qrelu_cases as Q
    return Q.bn_scaled(Q.bn_for(cout, seed=seed), var)


@pytest.mark.parametrize("fn", C.FNS)
def test_an_activation_read_by_a_conv_and_an_add(fn):
    """DUAL: the codes go to the conv, the float32 tensor of the same pass to the add."""
    spec = [_conv("quantized", 4, 3, 3, 8, 71), dict(_bn(8, 72, 3.0), dst="b0"), {"op": "act", "fn": fn, "nb": 4, "dst": "a0"},
            _conv("quantized", 4, 3, 8, 8, 73, src="a0"), dict(_bn(8, 74, 8.0), dst="b1"),
            {"op": "add", "a": "a0", "b": "b1", "dst": "s"}, {"op": "act", "fn": fn, "nb": 4},
            {"op": "flatten"}, S._dense("quantized", 4, 4 * 4 * 8, 10, 75)]
    x = np.random.default_rng(76).uniform(0, 1, (3, 4, 4, 3)).astype(F32)
    want = C.run_spec(spec, x)
    on, off = engine.GraphModel(spec, scaled_codes=True), engine.GraphModel(spec, scaled_codes=False)
    on.kernel_log = []
    got = host(on(dev(x)))
    assert C.same_bits(got, want) and C.same_bits(host(off(dev(x))), want)
    assert on.kernel_log == ["maxact_apply", "maxact_pack_i4", "generic_scaled", "maxact_pack_i4", "dense_i4_scaled"]


def test_an_8bit_activation_read_by_a_dense_layer_and_the_output_uses_the_dual_pack():
    """I8: the float32 tensor comes out of the pack's own pass."""
    fn = "quantized_leakymaxrelu"
    spec = [_conv("quantized", 8, 3, 3, 8, 77), dict(_bn(8, 78, 3.0), dst="b0"), {"op": "act", "fn": fn, "nb": 8, "dst": "a0"},
            {"op": "flatten", "src": "a0", "dst": "f"}, dict(S._dense("quantized", 8, 4 * 4 * 8, 8, 79), src="f", dst="d"),
            {"op": "flatten", "src": "a0", "dst": "g"}, dict(S._dense("float", 0, 4 * 4 * 8, 8, 80), src="g", dst="h"),
            {"op": "add", "a": "d", "b": "h"}]
    x = np.random.default_rng(76).uniform(0, 1, (3, 4, 4, 3)).astype(F32)
    on, off = engine.GraphModel(spec, scaled_codes=True), engine.GraphModel(spec, scaled_codes=False)
    on.kernel_log = []
    got = host(on(dev(x)))
    assert on.kernel_log == ["maxact_pack_i8_dual", "dense_i8_scaled"]
    assert np.isfinite(got).all() and C.same_bits(got, host(off(dev(x))))


@pytest.mark.parametrize("fn", C.FNS)
def test_a_vgg_shaped_network_takes_the_matrix_pipe(fn):
    """conv - BN - act - conv with 64 -> 128 channels: where the log without scaled_codes has the generic float32 kernel, the
    log with it has the pack and the scaled tile kernel of qnn_route_gemm."""
    spec = [_conv("quantized", 4, 3, 3, 64, 101), _bn(64, 102, 3.0), {"op": "act", "fn": fn, "nb": 4},
            _conv("quantized", 4, 3, 64, 128, 103), _bn(128, 104, 60.0), {"op": "act", "fn": fn, "nb": 4},
            {"op": "flatten"}, S._dense("quantized", 4, 4 * 4 * 128, 10, 105)]
    x = np.random.default_rng(106).uniform(0, 1, (3, 4, 4, 3)).astype(F32)
    want = C.run_spec(spec, x)
    on, off = engine.GraphModel(spec, scaled_codes=True), engine.GraphModel(spec, scaled_codes=False)
    on.kernel_log = []
    assert C.same_bits(host(on(dev(x))), want) and C.same_bits(host(off(dev(x))), want)
    assert on.kernel_log == ["maxact_pack_i4", "mfma_i4_256x128_scaled", "maxact_pack_i4", "dense_i4_scaled"]
    wf = engine._prepack(spec[3], _abi.STORE_F32, CUDA)
    _abi.conv2d(wf, dev(np.zeros((3, 4, 4, 64), F32)), _abi.STORE_F32, 0, 3, 4, 4)
    assert _abi.last_kernel() == "mfma_f32_act_c64"              # what the float32 route runs for this layer (64 input channels)


def test_a_consumer_beyond_the_bound_stays_on_the_float_route():
    """8 / 8 bits: the 3x3 conv over 128 channels has K = 1152 > 1024 and keeps the float32 route; the dense layer behind the
    next activation (K = 4 * 4 * 8 = 128) takes the scaled one."""
    fn = "quantized_maxrelu"
    spec = [_conv("quantized", 8, 3, 3, 128, 81), _bn(128, 82, 3.0), {"op": "act", "fn": fn, "nb": 8},
            _conv("quantized", 8, 3, 128, 8, 83), _bn(8, 84, 100.0), {"op": "act", "fn": fn, "nb": 8},
            {"op": "flatten"}, S._dense("quantized", 8, 4 * 4 * 8, 10, 85)]
    assert not engine.scaled_route_exact(1152, 8, 8) and engine.scaled_route_exact(128, 8, 8)
    x = np.random.default_rng(86).uniform(0, 1, (3, 4, 4, 3)).astype(F32)
    on, off = engine.GraphModel(spec, scaled_codes=True), engine.GraphModel(spec, scaled_codes=False)
    on.kernel_log = []
    got = host(on(dev(x)))
    assert on.kernel_log == ["maxact_pack_i8", "dense_i8_scaled"]
    assert np.isfinite(got).all() and C.same_bits(got, host(off(dev(x))))
