"""quantized_maxrelu / quantized_leakymaxrelu on the GPU, bit for bit against the numpy restatement of the contract
(maxrelu_cases.py, which test_maxrelu_cpu.py holds against golden/ref_maxrelu.npz): the reference's vectors, the sizes and
positions at which a reduction goes wrong, in place, the two halves, a reused workspace, the NaN rule, the valid rows of
a padded shard, what the other entries refuse, and two small networks through GraphModel and Model.predict."""

import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine, nets, shard
from oracle import qnn_oracle as O
import maxrelu_cases as C
import qrelu_cases as Q

pytestmark = pytest.mark.gpu
F32 = np.float32
CUDA = torch.device("cuda")
FN = {"quantized_maxrelu": _abi.FN_QUANTIZED_MAXRELU, "quantized_leakymaxrelu": _abi.FN_QUANTIZED_LEAKYMAXRELU}
OP = {"quantized_maxrelu": engine.quantized_ops.quantized_maxrelu,
      "quantized_leakymaxrelu": engine.quantized_ops.quantized_leakymaxrelu}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _workspace():
    return torch.full((4,), 0x55555555, dtype=torch.int32, device=CUDA)      # garbage: the entry clears it itself


def _one_call(x, y, fn, nb, ws):
    _abi.check(_abi.load().qnn_quantized_maxact_f32(_abi.ptr(x), _abi.ptr(y), x.numel(), FN[fn], nb, _abi.ptr(ws),
                                                    _abi.stream_ptr()), "qnn_quantized_maxact_f32")


# ---- the op against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", C.NBS)
@pytest.mark.parametrize("fn", C.FNS)
def test_the_reference_vectors(fn, nb):
    for ci in range(len(C.MAXIMA)):
        x, mx, lk = C.fixture(nb, ci)
        want = mx if fn == "quantized_maxrelu" else lk
        got = host(OP[fn](dev(x), nb))
        assert C.same_bits(got, want), (ci, np.count_nonzero(got.view(np.int32) != want.view(np.int32)))
    # the band where the reference depends on its log: the exact rule, whatever the reference recorded
    for i in range(len(C.AMBIGUOUS)):
        x = C.fixture_ambiguous(nb, i)[0]
        assert C.same_bits(host(OP[fn](dev(x), nb)), C.maxact(x, nb, fn)), float(C.AMBIGUOUS[i])


# the last size is the only one at which k_maxact_reduce's unrolled loop runs: it takes four float4 per lane, a grid
# stride (1024 blocks x 256 lanes) apart, and needs more than 3 x 2^18 float4; below that the remainder loop does the walk
STRIDE4 = 1024 * 256
SIZES = (1, 3, 4, 5, 255, 256, 257, 1027, 2 ** 20 + 7, 4 * 2 ** 20 + 7)
_base = {}


def _noise(n):
    """n values in [-3, 0.9) (one array, sliced): every maximum a test plants is 1.3, so a reduction that misses the
    planted element scales by 1 instead of 2."""
    if "x" not in _base:
        _base["x"] = np.random.default_rng(7).uniform(-3.0, 0.9, max(SIZES)).astype(F32)
    return _base["x"][:n].copy()


def _positions(n):
    """Index 0, the last element (inside the n % 4 tail), both sides of the first block boundary (256 lanes x 4 values),
    and -- past 1024 blocks x 256 lanes x 4 values -- the capped grid's second round, whose last block is its first."""
    pos = {p for p in (0, n - 1, 1023, 1024, 2 ** 20 - 1, 2 ** 20 + 1) if 0 <= p < n}
    if n // 4 > 3 * STRIDE4:
        # each of the four unrolled slots (float4 i + u * stride, for a lane in the middle of a block and for the grid's
        # last lane), the remainder loop's float4 behind them, and the tail
        for i4 in (1000, STRIDE4 - 1):
            pos |= {4 * (i4 + u * STRIDE4) + (u + 1) % 4 for u in range(4)}
        pos |= {4 * 4 * STRIDE4 + 2, n - 2}
        assert 4 * 4 * STRIDE4 + 2 < (n // 4) * 4 <= n - 2
    return sorted(pos)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_the_place_of_the_maximum(n):
    nb = 4
    for pos in _positions(n):
        x = _noise(n)
        x[pos] = F32(1.3)
        xd = dev(x)
        for fn in C.FNS:
            want = C.maxact(x, nb, fn)
            assert want[pos] == F32(1.25) and np.isfinite(want).all()
            got = host(OP[fn](xd, nb))
            assert C.same_bits(got, want), (n, pos, fn, np.count_nonzero(got != want))
    # in place, and the two halves against the one-call entry; a reused workspace must not keep the larger maximum
    x = _noise(n)
    x[n // 2] = F32(1.3)
    lib = _abi.load()
    for fn in C.FNS:
        want = C.maxact(x, nb, fn)
        ws = _workspace()
        y = torch.empty(n, dtype=torch.float32, device=CUDA)
        _one_call(dev(x), y, fn, nb, ws)
        assert C.same_bits(host(y), want)
        assert host(ws).tolist() == [int(F32(1.3).view(np.int32)), 0, 0, 0]
        xin = dev(x)
        _one_call(xin, xin, fn, nb, ws)
        assert C.same_bits(host(xin), want), "in place"
        small = (x * F32(0.25)).astype(F32)                     # maximum 0.325: scale 0.5 on the SAME workspace
        _one_call(dev(small), y, fn, nb, ws)
        assert C.same_bits(host(y), C.maxact(small, nb, fn)), "stale workspace"
        ws2, y2, xd = _workspace(), torch.empty(n, dtype=torch.float32, device=CUDA), dev(x)
        _abi.check(lib.qnn_maxact_max_f32(_abi.ptr(xd), n, _abi.ptr(ws2), _abi.stream_ptr()), "qnn_maxact_max_f32")
        _abi.check(lib.qnn_maxact_apply_f32(_abi.ptr(xd), _abi.ptr(y2), n, FN[fn], nb, _abi.ptr(ws2), _abi.stream_ptr()),
                   "qnn_maxact_apply_f32")
        assert C.same_bits(host(y2), want), "split halves"


@pytest.mark.parametrize("fn", C.FNS)
def test_wide_codes_and_the_ends_of_the_exact_range(fn):
    for nb, M in ((24, 1.3), (16, 2.0 ** 64), (2, 2.0 ** -64), (24, 2.0 ** -64), (24, 1.3 * 2.0 ** 63), (3, 1.3 * 2.0 ** -64)):
        x = (_noise(1027).astype(np.float64) * (M / 1.3)).astype(F32)            # below 0.7 M
        x[5] = F32(M)
        want = C.maxact(x, nb, fn)
        assert np.isfinite(want).all() and want[5] > 0
        assert C.same_bits(host(OP[fn](dev(x), nb)), want), (nb, M)
    x = np.array([2.0 ** -65 * 1.0001, -1.0, 0.0, 2.0 ** -66], F32)        # still P = 2^-64: exact
    assert C.same_bits(host(OP[fn](dev(x), 4)), C.maxact(x, 4, fn)) and np.isfinite(C.maxact(x, 4, fn)).all()
    for M in (2.0 ** 64 * 1.0001, 2.0 ** -65, 1e-40, np.inf):             # outside it: NaN everywhere, as the header says
        x = np.array([M, -M, 0.0, M / 2, M / 4], F32)
        assert np.isnan(C.maxact(x, 4, fn)).all() and np.isnan(host(OP[fn](dev(x), 4))).all(), M


@pytest.mark.parametrize("fn", C.FNS)
def test_no_positive_value_gives_nan_everywhere(fn):
    for n in (1, 5, 1027):
        for x in (np.zeros(n, F32), -np.zeros(n, F32), -np.abs(_noise(n)) - F32(0.5)):
            got = host(OP[fn](dev(x), 4))
            assert got.shape == x.shape and np.isnan(got).all()
            assert np.array_equal(got.view(np.uint32), np.full(n, 0x7FC00000, np.uint32))       # the quiet NaN
    torch.cuda.synchronize()                                     # and the device is in order
    x = _noise(257)
    x[3] = F32(1.3)
    assert C.same_bits(host(OP[fn](dev(x), 4)), C.maxact(x, 4, fn))


@pytest.mark.parametrize("fn", C.FNS)
def test_valid_rows_keep_the_padding_out_of_the_maximum(fn):
    x = _noise(6 * 35).reshape(6, 5, 7)
    x[1, 2, 3] = F32(1.3)
    x[4:] = F32(5.0)                                             # the padded rows carry a larger value: it must not win
    want = C.maxact(x, 4, fn, M=F32(1.3))
    assert not C.same_bits(want, C.maxact(x, 4, fn))
    with shard.sharded(None, valid_rows=4):
        got = host(OP[fn](dev(x), 4))
    assert C.same_bits(got, want)                                # every row is scaled, the padded ones clip at the top code
    assert C.same_bits(host(OP[fn](dev(x), 4)), C.maxact(x, 4, fn))      # outside the context every row counts
    with shard.sharded(None, valid_rows=0):                      # an empty shard of one process: no maximum at all
        assert np.isnan(host(OP[fn](dev(x), 4))).all()


# ---- refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", C.FNS)
def test_every_other_entry_refuses_the_two_functions(fn):
    N, H, W, cin, cout = 2, 5, 7, 8, 16
    op = Q.conv_op("quantized", 4, 3, cin, cout, 1, seed=41)
    w = engine._prepack(op, _abi.STORE_I4, CUDA, stride=1, same_pad=True)
    xg = Q.grid_values((N, H, W, cin), 4, seed=42)
    xp = _abi.pack(dev(xg), cin, _abi.FN_GRID, 4, _abi.STORE_I4)
    named = "qnn_quantized_maxact_f32"
    with pytest.raises(_abi.QnnUnsupported, match=named):
        _abi.pack(dev(xg), cin, FN[fn], 4, _abi.STORE_I4)
    for out_store in (_abi.STORE_I4, _abi.STORE_F32):
        with pytest.raises(_abi.QnnUnsupported, match=named):
            _abi.conv2d(w, xp, _abi.STORE_I4, 4, N, H, W, fn=FN[fn], act_bits=4, out_store=out_store)
    wf = engine._prepack(op, _abi.STORE_F32, CUDA, stride=1, same_pad=True)
    with pytest.raises(_abi.QnnUnsupported, match=named):
        _abi.conv2d(wf, dev(xg), _abi.STORE_F32, 0, N, H, W, fn=FN[fn], act_bits=4)
    with pytest.raises(_abi.QnnUnsupported, match=named):
        _abi.conv2d_f32in(w, dev(xg), FN[fn], 4)
    with pytest.raises(_abi.QnnUnsupported, match=named):
        _abi.conv2d_f32in(w, dev(xg), _abi.FN_QUANTIZED_TANH, 4, fn=FN[fn], act_bits=4, out_store=_abi.STORE_I4)
    dk = {"op": "dense", "kind": "quantized", "nb": 4, "kernel": np.random.default_rng(43).uniform(-1, 1, (64, 10)).astype(F32),
          "bias": None}
    xd = Q.grid_values((6, 64), 4, seed=44)
    with pytest.raises(_abi.QnnUnsupported, match=named):
        _abi.dense(engine._prepack(dk, _abi.STORE_I4, CUDA), _abi.pack(dev(xd), 64, _abi.FN_GRID, 4, _abi.STORE_I4),
                   _abi.STORE_I4, 4, 6, fn=FN[fn], act_bits=4)
    with pytest.raises(_abi.QnnUnsupported, match=named):
        _abi.dense(engine._prepack(dk, _abi.STORE_F32, CUDA), dev(xd), _abi.STORE_F32, 0, 6, fn=FN[fn], act_bits=4)
    # a layer qnn_fold_prepare folds for quantized_tanh
    op16 = Q.conv_op("quantized", 4, 3, 16, 16, 1, seed=45)
    w16 = engine._prepack(op16, _abi.STORE_I4, CUDA, stride=1, same_pad=True)
    inv, shift = (dev(a) for a in engine.bn_constants(Q.bn_scaled(Q.bn_for(16, seed=46), 9 * 16 * 0.1)))
    assert _abi.Fold.try_prepare(w16, _abi.STORE_I4, 4, inv, shift, _abi.FN_QUANTIZED_TANH, 4, _abi.STORE_I4) is not None
    with pytest.raises(_abi.QnnUnsupported, match=named):
        _abi.Fold(w16, _abi.STORE_I4, 4, inv, shift, FN[fn], 4, _abi.STORE_I4)
    # and quantized_tanh calls still take the kernels they took
    x16 = Q.grid_values((2, 7, 20, 16), 4, seed=47)
    y, _, _ = _abi.conv2d(w16, _abi.pack(dev(x16), 16, _abi.FN_GRID, 4, _abi.STORE_I4), _abi.STORE_I4, 4, 2, 7, 20, inv, shift,
                          _abi.FN_QUANTIZED_TANH, 4, 1, _abi.STORE_I4)
    assert _abi.last_kernel() == "strip_i4_c16"
    y, _, _ = _abi.conv2d(w, xp, _abi.STORE_I4, 4, N, H, W, fn=_abi.FN_QUANTIZED_TANH, act_bits=4, out_store=_abi.STORE_I4)
    want = O.quantized_tanh(O.quantized_conv2d_call(xg, op["kernel"], op["bias"], 4, None, (1, 1), "same"), 4)
    assert np.array_equal(host(_abi.unpack(y, N * H * W, cout, _abi.STORE_I4, 4)).reshape(want.shape), want)
    xt = _noise(1027)
    assert np.array_equal(host(engine.quantized_ops.quantized_tanh(dev(xt), 4)), O.quantized_tanh(xt, 4))


# ---- whole networks ------------------------------------------------------------------------------------------------------
_nets = {}


def _net(arch, nt, fn):
    """The small networks of test_gpu_qrelu.py with the activation replaced, 3 images, and their numpy runs: the whole
    batch at once, and in batches of 2 (each batch scaled by its own maxima)."""
    if (arch, nt, fn) not in _nets:
        kw = dict(network_type=nt, wbits=4, abits=4)
        if arch == "RESNET":
            # 16 x 16 images leave a 4 x 4 map in front of the classifier: the pool covers the whole map (size 4)
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


def _same(got, want, what):
    """Bit for bit: every convolution's sums are exact or reproduced.  Behind the first layer the activations are P k / m and
    the weights low-bit codes, so every partial sum is an integer below 2^24 times a power of two; the first layer sums
    float32 images in the device kernels' order, which the oracle's "device" order restates (as for the same networks in
    test_gpu_qrelu.py).  No network here has a layer with float weights, so the band for float paths applies nowhere."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(want).all(), what
    print("%s: max |diff| %.3g, %d of %d values differ" % (what, np.abs(got - want).max(), np.count_nonzero(got != want), got.size))
    assert C.same_bits(got, want), what


@pytest.mark.parametrize("fn", C.FNS)
@pytest.mark.parametrize("nt", ["full-qnn", "qbnn"])
@pytest.mark.parametrize("arch", ["RESNET", "VGG"])
def test_whole_networks(arch, nt, fn):
    cf, spec, x, want, want2 = _net(arch, nt, fn)
    xd = dev(x)
    assert want.shape == want2.shape == (3, 10)
    for cls in (engine.FusedModel, engine.ResidualFusedModel):
        with pytest.raises(_abi.NotFusable, match="maximum of the whole batch"):
            cls(spec)
    g = engine.GraphModel(spec)
    got = host(g(xd))
    _same(got, want, "GraphModel")
    assert np.array_equal(host(g(xd)), got)
    _same(host(engine.LayerModel(spec)(xd)), want, "LayerModel")
    # Model.predict: full batches replayed from hipGraphs and a ragged tail, each batch with its own maximum
    model = nets.Model(cf, spec)
    assert isinstance(model.engine, engine.GraphModel)
    first = model.predict(x, batch_size=2)
    _same(first, want2, "Model.predict(batch_size=2)")
    assert np.array_equal(model.predict(x, batch_size=2), first)              # the captured graphs, replayed
    assert np.array_equal(host(model.predict(xd, batch_size=2)), first)
    _same(host(g(xd[:2])), want2[:2], "GraphModel, first two images")
