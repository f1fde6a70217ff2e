"""Channel concatenation on the GPU (include/qnn_abi_concat.h, csrc/qnn_concat.hip) against the numpy reference of
concat_cases.py, bit for bit, with the kernel name asserted: every channel list of the case table at every pixel count and
code width, with the inputs' spare bits set, with every pointer moved off its 16-byte alignment, and one input alone; the
packed result as the input of a convolution; the layer class; the op on GraphModel, captured and replayed; the refusals of
the other engines.

The kernel forms (concat_cases.form; the name qnn_last_kernel() gives is per store, so the form is the host's rule
restated): k_concat_words<4> runs the lists of ALIGNED, k_concat_words<1> those of WORD, the ALIGNED ones once their
pointers are off 16 bytes, and every float32 list but [4, 4]; k_concat_funnel<1> every other BIN / I4 / I8 list,
k_concat_funnel<2> both T2 lists."""
import ctypes

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi, engine, nets

import concat_cases as C

pytestmark = pytest.mark.gpu
F32 = np.float32
FILL = 0x5A5A5A5A
ENTRY = _abi.EXPORTS_CONCAT[0]           # read at import: without the entry, the op and the class nothing below means anything
LAYER = qnn_amd.Concatenate


def dev(a):
    a = np.array(a, order="C")               # a writable copy: the case tables are read-only
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host(t):
    torch.cuda.synchronize()
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def bits_of(a):
    return np.ascontiguousarray(a).view(np.uint32)


def inputs(kind, bits, pixels, channels, dirty=False):
    """The inputs of one call as numpy words (float32: values): [(pixels, words)]."""
    if kind == "f32":
        return [C.f32_values(pixels, c, i) for i, c in enumerate(channels)]
    ws = [C.encode(C.codes(kind, bits, pixels, c, i), kind) for i, c in enumerate(channels)]
    return [w | C.spare(kind, c) for w, c in zip(ws, channels)] if dirty else ws


def off_by_a_word(a):
    """A device copy of `a` whose address is 4 bytes past a 16-byte boundary."""
    t = dev(a)
    buf = torch.full((t.numel() + 4,), FILL, dtype=torch.int32, device="cuda").view(t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v, buf


def raw(xs, channels, kind, bits, pixels, y):
    """qnn_concat_forward on the caller's own output tensor."""
    d = _abi.Concat()
    d.n = len(xs)
    for i, (t, c) in enumerate(zip(xs, channels)):
        d.channels[i] = c
        d.x[i] = t.data_ptr()
    _abi.check(_abi.load().qnn_concat_forward(ctypes.byref(d), C.STORE[kind], bits, pixels, _abi.ptr(y), _abi.stream_ptr()),
               "qnn_concat_forward")
    return y


CASES = [(kind, i) for kind in ("bin", "i4", "i8", "t2", "f32") for i in range(len(C.LISTS[kind]))]


@pytest.mark.parametrize("kind,li", CASES, ids=["%s-%s" % (k, "_".join(map(str, C.LISTS[k][i]))) for k, i in CASES])
def test_concat_of_every_list(kind, li):
    channels = C.LISTS[kind][li]
    store, total = C.STORE[kind], sum(channels)
    for pixels in C.PIXELS:
        for bits in C.BITS[kind]:
            clean = inputs(kind, bits, pixels, channels)
            want = bits_of(C.concat_ref(clean, channels, kind))
            assert want.shape == (pixels, C.words(kind, total))
            got = host(_abi.concat([dev(w) for w in clean], channels, store, bits, pixels))
            assert _abi.last_kernel() == "concat_" + kind
            np.testing.assert_array_equal(bits_of(got), want, err_msg="%s %s pixels=%d bits=%d" % (kind, channels, pixels, bits))
            if kind != "f32":
                # every input's spare bits set to ones: the same words, the output's own spare bits zero
                dirty = inputs(kind, bits, pixels, channels, dirty=True)
                got = host(_abi.concat([dev(w) for w in dirty], channels, store, bits, pixels))
                np.testing.assert_array_equal(got, want, err_msg="spare bits %s %s pixels=%d" % (kind, channels, pixels))
                assert not np.any(got & C.spare(kind, total))
            # every pointer one word past a 16-byte boundary: the one-word forms, the same bits
            moved = [off_by_a_word(w) for w in (clean if kind == "f32" else inputs(kind, bits, pixels, channels, dirty=True))]
            y, ybuf = off_by_a_word(np.full(want.shape, FILL, dtype=np.uint32))
            raw([v for v, _ in moved], channels, kind, bits, pixels, y)
            assert _abi.last_kernel() == "concat_" + kind
            np.testing.assert_array_equal(host(y), want, err_msg="moved pointers %s %s pixels=%d" % (kind, channels, pixels))
            edge = host(ybuf)
            assert edge[0] == FILL and np.all(edge[1 + want.size:] == FILL)      # nothing written around y
            # one input: a copy with the spare bits cleared
            one = inputs(kind, bits, pixels, channels[:1], dirty=kind != "f32")
            got = host(_abi.concat([dev(one[0])], channels[:1], store, bits, pixels))
            np.testing.assert_array_equal(bits_of(got), bits_of(C.concat_ref(one, channels[:1], kind)))
            assert _abi.last_kernel() == "concat_" + kind


def test_inputs_and_output_side_by_side_in_one_buffer():
    """y begins where the last input ends: no overlap, and the call writes y alone."""
    channels, pixels = [12, 24, 36], 7
    ws = inputs("i4", 4, pixels, channels)
    sizes = [w.size for w in ws]
    nout = pixels * C.words("i4", sum(channels))
    buf = torch.full((sum(sizes) + nout + 8,), FILL, dtype=torch.int32, device="cuda")
    xs, at = [], 0
    for w in ws:
        v = buf[at:at + w.size].view(w.shape)
        v.copy_(dev(w))
        xs.append(v)
        at += w.size
    y = buf[at:at + nout].view(pixels, -1)
    raw(xs, channels, "i4", 4, pixels, y)
    np.testing.assert_array_equal(host(y), C.concat_ref(ws, channels, "i4"))
    for v, w in zip(xs, ws):
        np.testing.assert_array_equal(host(v), w)
    assert np.all(host(buf[at + nout:]) == FILL)
    with pytest.raises(_abi.QnnError, match="overlap"):
        raw(xs, channels, "i4", 4, pixels, buf[at - 1:at - 1 + nout].view(pixels, -1))


@pytest.mark.parametrize("kind,bits,channels", [("bin", 1, [31, 1, 33]), ("i4", 4, [12, 24, 36]), ("i4", 3, [7, 9, 16]),
                                                ("i8", 8, [3, 64]), ("i8", 5, [1, 2, 5]), ("t2", 1, [32, 31]), ("i4", 4, [32, 64])])
def test_concat_of_packs_is_pack_of_the_concatenation(kind, bits, channels):
    store, pixels = C.STORE[kind], 35
    m = 1.0 if kind in ("bin", "t2") else float(1 << (bits - 1))
    vals = [(C.codes(kind, bits, pixels, c, 10 + i) / m).astype(F32) for i, c in enumerate(channels)]
    packs = [_abi.pack(dev(v), c, _abi.FN_GRID, bits, store) for v, c in zip(vals, channels)]
    got = _abi.concat(packs, channels, store, bits, pixels)
    assert _abi.last_kernel() == "concat_" + kind
    want = _abi.pack(dev(np.concatenate(vals, axis=-1)), sum(channels), _abi.FN_GRID, bits, store)
    assert torch.equal(got, want)
    back = _abi.unpack(got, pixels, sum(channels), store, bits)
    np.testing.assert_array_equal(host(back), np.concatenate(vals, axis=-1))


@pytest.mark.parametrize("channels", [[12, 12], [8, 16], [3, 5, 16]])
def test_the_packed_result_feeds_a_convolution(channels):
    """conv(concat of the packed codes) == conv(float32 concat), bit for bit: dyadic operands, every sum exact."""
    N, H, W, cin = 2, 5, 4, sum(channels)
    rng = np.random.default_rng(7)
    op = {"op": "conv", "kind": "quantized", "nb": 4, "kernel": (rng.integers(-8, 8, (3, 3, cin, 16)) / 8.0).astype(F32), "bias": None}
    vals = [(C.codes("i4", 4, N * H * W, c, 20 + i) / 8.0).astype(F32) for i, c in enumerate(channels)]
    packs = [_abi.pack(dev(v), c, _abi.FN_GRID, 4, _abi.STORE_I4) for v, c in zip(vals, channels)]
    xp = _abi.concat(packs, channels, _abi.STORE_I4, 4, N * H * W)
    y_codes = _abi.conv2d(engine._prepack(op, _abi.STORE_I4, "cuda"), xp, _abi.STORE_I4, 4, N, H, W)[0]
    xf = _abi.concat([dev(v) for v in vals], channels, _abi.STORE_F32, 0, N * H * W)
    assert _abi.last_kernel() == "concat_f32"
    np.testing.assert_array_equal(host(xf), np.concatenate(vals, axis=-1))
    y_f32 = _abi.conv2d(engine._prepack(op, _abi.STORE_F32, "cuda"), xf.reshape(N, H, W, cin), _abi.STORE_F32, 0, N, H, W)[0]
    assert y_codes.shape == y_f32.shape == (N, H, W, 16)
    assert torch.equal(y_codes, y_f32) and float(y_f32.abs().max()) > 0


def test_the_layer_class():
    xs = [C.f32_values(2 * 7 * 20, c, 30 + i).reshape(2, 7, 20, c) for i, c in enumerate((3, 5, 4))]
    for axis in (-1, 3):
        y = qnn_amd.Concatenate(axis=axis)([dev(x) for x in xs])
        assert _abi.last_kernel() == "concat_f32" and y.shape == (2, 7, 20, 12) and y.dtype == torch.float32
        np.testing.assert_array_equal(bits_of(host(y)), bits_of(np.concatenate(xs, axis=-1)))
    flat = [C.f32_values(5, c, 40 + i) for i, c in enumerate((10, 3))]
    for axis in (-1, 1):
        y = qnn_amd.Concatenate(axis=axis)([dev(x) for x in flat])
        np.testing.assert_array_equal(bits_of(host(y)), bits_of(np.concatenate(flat, axis=-1)))
    a, b = dev(xs[0]), dev(xs[1])
    with pytest.raises(_abi.QnnError, match="axis=1"):
        qnn_amd.Concatenate(axis=1)([a, b])
    with pytest.raises(ValueError, match="at least 2 inputs"):
        qnn_amd.Concatenate()([a])
    with pytest.raises(ValueError, match="matching shapes"):
        qnn_amd.Concatenate()([a, b[:, :6]])
    with pytest.raises(_abi.QnnError, match="9 inputs"):
        qnn_amd.Concatenate()([a] * 9)
    with pytest.raises(_abi.QnnError, match="no CPU path"):
        qnn_amd.Concatenate()([a, b.cpu()])
    nine = [C.f32_values(7, 1, 50 + i) for i in range(9)]          # the engines' helper joins more than eight in two calls
    log = []
    y = engine._concat_f32([dev(x) for x in nine], log)
    assert log == ["concat_f32", "concat_f32"]
    np.testing.assert_array_equal(bits_of(host(y)), bits_of(np.concatenate(nine, axis=-1)))


# ---- the spec op ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.SPECS))
def test_graph_model_runs_the_concat(name):
    net, log = C.SPECS[name]
    x = net.images()
    assert C.guard(net.spec, x) is None
    m = engine.GraphModel(net.spec)
    m.kernel_log = []
    got = host(m(dev(x)))
    assert m.kernel_log == log, m.kernel_log
    np.testing.assert_array_equal(got, C.reference(net.spec, x))
    assert np.unique(got).size > 10                      # (not a constant network)


def test_graph_model_keeps_the_codes_and_the_clips():
    """What the concat hands on: packed codes from packed branches (the conv behind reads them as they are), one clip
    over the joined pre-activations from two clips (materialised, it is the concatenation of the activations)."""
    m = engine.GraphModel(C.SPECS["packed_i4"][0].spec)
    a = engine._Packed(dev(C.encode(C.codes("i4", 4, 32, 12, 1), "i4")), _abi.STORE_I4, 4, (2, 4, 4, 12))
    b = engine._Packed(dev(C.encode(C.codes("i4", 4, 32, 12, 2), "i4")), _abi.STORE_I4, 4, (2, 4, 4, 12))
    y = m._concat([a, b])
    assert isinstance(y, engine._Packed) and (y.store, y.bits, y.shape) == (_abi.STORE_I4, 4, (2, 4, 4, 24))
    np.testing.assert_array_equal(host(y.t), C.concat_ref([host(a.t), host(b.t)], [12, 12], "i4"))
    b8 = engine._Packed(b.t, _abi.STORE_I4, 3, b.shape)                      # another width: joined in float32
    assert isinstance(m._concat([a, b8]), torch.Tensor)
    op = {"op": "act", "fn": "quantized_tanh", "nb": 4}
    pa = dev(np.linspace(-1.5, 1.5, 2 * 4 * 4 * 12, dtype=F32).reshape(2, 4, 4, 12))
    pb = dev(np.full((2, 4, 4, 5), -2.0, F32))
    va, vb = engine._Virtual(pa, _abi.FN_QUANTIZED_TANH, 4, op), engine._Virtual(pb, _abi.FN_QUANTIZED_TANH, 4, op)
    y = m._concat([va, vb])
    assert isinstance(y, engine._Virtual) and (y.fn, y.nb) == (_abi.FN_QUANTIZED_TANH, 4) and y.pre.shape == (2, 4, 4, 17)
    assert torch.equal(y.materialize(), torch.cat([va.materialize(), vb.materialize()], dim=-1))
    v2 = engine._Virtual(pb, _abi.FN_QUANTIZED_TANH, 2, {"op": "act", "fn": "quantized_tanh", "nb": 2})
    y = m._concat([va, v2])                                                  # another width: each clip applied, then joined
    assert isinstance(y, torch.Tensor) and torch.equal(y, torch.cat([va.materialize(), v2.materialize()], dim=-1))


def test_model_predict_replays_the_captured_graph():
    net = C.SPECS["densenet"][0]
    x = (np.random.default_rng(78).integers(0, 9, (4, 8, 8, 3)) / 8.0).astype(F32)
    assert C.guard(net.spec, x) is None
    cf = nets.Config(network_type="full-qnn", wbits=4, abits=4, architecture="RESNET", nres=1, dim=8)
    model = nets.Model(cf, net.spec)
    assert isinstance(model.engine, engine.GraphModel)           # the fused engines refuse the op, the model falls through
    xd = dev(x)
    first = host(model.predict(xd, batch_size=2))                # two full batches: captured, then replayed
    pipe = model.pipeline(2)
    assert len(pipe._lanes) == 1 and all("graph" in ln for lanes in pipe._lanes.values() for ln in lanes)
    second = host(model.predict(xd, batch_size=2))               # the same graphs, replayed again
    assert len(pipe._lanes) == 1
    want = C.reference(net.spec, x)
    np.testing.assert_array_equal(first, want)
    np.testing.assert_array_equal(second, want)
    np.testing.assert_array_equal(model.predict(x, batch_size=2), want)      # a host array, the same route
    pipe.clear()


@pytest.mark.parametrize("name", list(C.SPECS))
def test_the_other_engines_refuse_by_name(name):
    spec = C.SPECS[name][0].spec
    for cls in (engine.FusedModel, engine.ResidualFusedModel, engine.LayerModel):
        with pytest.raises(_abi.NotFusable, match="concat"):
            cls(spec)
