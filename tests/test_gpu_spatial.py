"""ZeroPadding2D, Cropping2D and UpSampling2D on the GPU (include/qnn_abi_spatial.h, csrc/qnn_spatial.hip) against the
numpy reference of spatial_cases.py, bit for bit, with the kernel name asserted: every descriptor of the case table on every
store, channel count and code width, with the input's spare bits set and with both pointers moved off their 16-byte
alignment; the identity and the empty batch; the layer classes; the ops on GraphModel and LayerModel, captured and replayed.

The kernel forms (spatial_cases.form; the name qnn_last_kernel() gives is per store, so the form is the host's rule
restated): 16 bytes per lane runs the last channel count of every store (and the 33 ternary channels: two word pairs with a
ragged last pair), 4 bytes per lane the others and the 16-byte ones once their pointers are off 16 bytes."""
import ctypes

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi, engine

import spatial_cases as Z

pytestmark = pytest.mark.gpu
F32 = np.float32
FILL = 0x5A5A5A5A
ENTRIES = _abi.EXPORTS_SPATIAL           # read at import: without the entries, the ops and the classes nothing below means anything
LAYERS = (qnn_amd.ZeroPadding2D, qnn_amd.Cropping2D, qnn_amd.UpSampling2D)


def dev(a):
    a = np.array(a, order="C")               # a writable copy: the case tables are read-only
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host(t):
    torch.cuda.synchronize()
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def bits_of(a):
    return np.ascontiguousarray(a).view(np.uint32)


def stored(kind, bits, shape, seed, dirty=False):
    """One input as numpy words (pixels, words) (float32: values (pixels, C))."""
    N, H, W, Cn = shape
    if kind == "f32":
        return Z.f32_values(N * H * W, Cn, seed)
    w = Z.encode(Z.codes(kind, bits, N * H * W, Cn, seed), kind)
    return w | Z.spare(kind, Cn) if dirty else w


def off_by_a_word(a):
    """A device copy of `a` whose address is 4 bytes past a 16-byte boundary."""
    t = dev(a)
    buf = torch.full((t.numel() + 4,), FILL, dtype=torch.int32, device="cuda").view(t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v, buf


def raw(x, kind, bits, shape, d, y):
    """qnn_spatial2d_forward on the caller's own output tensor."""
    desc = _abi.spatial_desc(d["crop"], d["up"], d["pad"])
    _abi.check(_abi.load().qnn_spatial2d_forward(_abi.ptr(x), Z.STORE[kind], bits, *shape, ctypes.byref(desc), _abi.ptr(y),
                                                 _abi.stream_ptr()), "qnn_spatial2d_forward")
    return y


def run(x, kind, bits, shape, d):
    y, Ho, Wo = _abi.spatial2d(x, Z.STORE[kind], bits, *shape, crop=d["crop"], up=d["up"], pad=d["pad"])
    assert (Ho, Wo) == Z.out_hw(shape[1], shape[2], d)
    assert _abi.last_kernel() == "spatial_" + kind
    return y


def check_one(kind, bits, shape, d, what):
    N, H, W, Cn = shape
    clean = stored(kind, bits, shape, 1)
    want = bits_of(Z.spatial_ref(clean, kind, shape, d)).reshape(-1, Z.words(kind, Cn))
    got = host(run(dev(clean.reshape(shape) if kind == "f32" else clean), kind, bits, shape, d))
    np.testing.assert_array_equal(bits_of(got).reshape(want.shape), want, err_msg=what)
    x = clean
    if kind != "f32":
        # garbage in the input's spare bits: the same words, the output's own spare bits zero
        x = stored(kind, bits, shape, 1, dirty=True)
        got = host(run(dev(x), kind, bits, shape, d))
        np.testing.assert_array_equal(got, want, err_msg="spare bits " + what)
        assert not np.any(got & Z.spare(kind, Cn))
    if Z.form(kind, Cn) == "v4":
        # both pointers one word past a 16-byte boundary: the 4-byte form, the same bits, nothing written around y
        assert Z.form(kind, Cn, aligned16=False) == "v1"
        xv, _ = off_by_a_word(x)
        y, ybuf = off_by_a_word(np.full(want.shape, FILL, dtype=np.uint32))
        raw(xv, kind, bits, shape, d, y)
        assert _abi.last_kernel() == "spatial_" + kind
        np.testing.assert_array_equal(host(y), want, err_msg="moved pointers " + what)
        edge = host(ybuf)
        assert edge[0] == FILL and np.all(edge[1 + want.size:] == FILL)


GRID = [(kind, name) for kind in ("bin", "t2", "i4", "i8", "f32") for name, _, d in Z.DESCS
        if not (kind == "bin" and Z.padded(d))]


@pytest.mark.parametrize("kind,name", GRID, ids=["%s-%s" % g for g in GRID])
def test_every_descriptor_on_every_store(kind, name):
    (H, W), d = next((hw, d) for n, hw, d in Z.DESCS if n == name)
    for Cn in [c for c in Z.CHANNELS[kind] if c]:
        for bits in Z.BITS[kind]:
            check_one(kind, bits, (Z.N_GRID, H, W, Cn), d, "%s %s C=%d bits=%d" % (kind, name, Cn, bits))


@pytest.mark.parametrize("kind", ["bin", "t2", "i4", "i8", "f32"])
def test_a_ragged_last_workgroup(kind):
    H, W = Z.RAGGED_IMAGE
    for name, _, d in Z.DESCS:
        if name in ("up23", "all") and not (kind == "bin" and Z.padded(d)):
            for Cn in (Z.CHANNELS[kind][0], Z.CHANNELS[kind][2]):
                check_one(kind, Z.BITS[kind][0], (2, H, W, Cn), d, "%s %s 2x7x20x%d" % (kind, name, Cn))


@pytest.mark.parametrize("kind", ["bin", "t2", "i4", "i8", "f32"])
def test_rows_longer_than_a_block(kind):
    """300 output pixels a row: a block strides along the row (several chunks, the last one ragged), one row per block."""
    d = Z.desc(crop=((0, 0), (1, 0)), up=(2, 3), pad=((0, 0), (0, 0) if kind == "bin" else (2, 1)))
    for Cn in (Z.CHANNELS[kind][0], Z.CHANNELS[kind][2]):
        check_one(kind, Z.BITS[kind][0], (2, 2, 101, Cn), d, "%s 2x2x101x%d" % (kind, Cn))


@pytest.mark.parametrize("kind", ["bin", "t2", "i4", "i8", "f32"])
def test_identity_and_empty_batch(kind):
    bits, Cn = Z.BITS[kind][0], Z.CHANNELS[kind][0]
    shape = (2, 3, 5, Cn)
    x = stored(kind, bits, shape, 4, dirty=True)
    got = host(run(dev(x.reshape(shape) if kind == "f32" else x), kind, bits, shape, Z.IDENTITY))
    if kind == "f32":
        np.testing.assert_array_equal(bits_of(got).reshape(-1), bits_of(x).reshape(-1))
    else:
        np.testing.assert_array_equal(got, x & ~Z.spare(kind, Cn))           # the input with its spare bits cleared
    # N == 0: no launch, the kernel name is not set again
    _abi.pool2d(torch.zeros(1, 2, 2, 1, device="cuda"), _abi.STORE_F32, 0, 1, 2, 2, 1, _abi.POOL_MAX, 2)
    before = _abi.last_kernel()
    empty = torch.empty((0, 3, 5, Cn), dtype=torch.float32, device="cuda") if kind == "f32" else \
        torch.empty((0, Z.words(kind, Cn)), dtype=torch.int32, device="cuda")
    y, Ho, Wo = _abi.spatial2d(empty, Z.STORE[kind], bits, 0, 3, 5, Cn, up=(2, 3))
    assert (Ho, Wo) == (6, 15) and y.numel() == 0 and _abi.last_kernel() == before
    if kind == "bin":
        with pytest.raises(_abi.QnnUnsupported, match="no zero.*unpack, pad in float32"):
            _abi.spatial2d(dev(x), _abi.STORE_BIN, 1, *shape, pad=((1, 0), (0, 0)))


def test_the_layer_classes_against_torch():
    x = Z.f32_values(2 * 4 * 6, 3, 9).reshape(2, 4, 6, 3)
    t, xd = torch.from_numpy(np.array(x)), dev(x)
    for pad in (1, (1, 2), ((1, 2), (0, 3))):
        (pt, pb), (pl, pr) = qnn_amd.ZeroPadding2D(pad).padding
        y = qnn_amd.ZeroPadding2D(pad)(xd)
        assert _abi.last_kernel() == "spatial_f32" and y.dtype == torch.float32
        np.testing.assert_array_equal(bits_of(host(y)), bits_of(torch.nn.functional.pad(t, (0, 0, pl, pr, pt, pb)).numpy()))
    for crop in (1, (1, 2), ((1, 0), (2, 1))):
        (ct, cb), (cl, cr) = qnn_amd.Cropping2D(crop).cropping
        y = qnn_amd.Cropping2D(crop)(xd)
        np.testing.assert_array_equal(bits_of(host(y)), bits_of(t[:, ct:4 - cb, cl:6 - cr].contiguous().numpy()))
    for size in (2, (2, 3), (1, 1)):
        uy, ux = qnn_amd.UpSampling2D(size).size
        y = qnn_amd.UpSampling2D(size)(xd)
        assert y.shape == (2, 4 * uy, 6 * ux, 3)
        np.testing.assert_array_equal(bits_of(host(y)), bits_of(t.repeat_interleave(uy, 1).repeat_interleave(ux, 2).numpy()))
    with pytest.raises(_abi.QnnError, match="no CPU path"):
        qnn_amd.UpSampling2D()(t)
    with pytest.raises(_abi.QnnError, match="no row"):
        qnn_amd.Cropping2D(2)(xd)
    with pytest.raises(ValueError, match="ndim=4"):
        qnn_amd.ZeroPadding2D()(xd[0])


# ---- the spec ops -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Z.SPECS))
def test_graph_model_moves_the_codes(name):
    """The encoder-decoder and the crop / pad network: between the clip and the next low-bit layer the activation is
    resized and joined on its codes, never unpacked."""
    net, log = Z.SPECS[name]
    x = net.images()
    assert x.shape[0] == 2 and Z.guard(net.spec, x) is None
    m = engine.GraphModel(net.spec)
    m.kernel_log = []
    got = host(m(dev(x)))
    assert m.kernel_log == log, m.kernel_log
    np.testing.assert_array_equal(got, Z.reference(net.spec, x))
    assert np.unique(got).size > 10                      # (not a constant network)


@pytest.mark.parametrize("name", list(Z.CHAINS))
def test_graph_model_and_layer_model_agree_with_the_reference(name):
    """The same networks without the concat (LayerModel reads one tensor per op and refuses that op by name)."""
    net, log = Z.CHAINS[name]
    x = net.images()
    assert Z.guard(net.spec, x) is None
    want = Z.reference(net.spec, x)
    m = engine.GraphModel(net.spec)
    m.kernel_log = []
    np.testing.assert_array_equal(host(m(dev(x))), want)
    assert m.kernel_log == log, m.kernel_log
    np.testing.assert_array_equal(host(engine.LayerModel(net.spec)(dev(x))), want)
    assert _abi.last_kernel() != "" and np.unique(want).size > 10


def test_a_binary_pad_runs_in_float32_and_a_binary_upsample_on_codes():
    for net, log in ((Z.binary_pad(), ["spatial_f32"]), (Z.binary_upsample(), ["spatial_bin"])):
        x = net.images()
        assert Z.guard(net.spec, x) is None
        m = engine.GraphModel(net.spec)
        m.kernel_log = []
        want = Z.reference(net.spec, x)
        np.testing.assert_array_equal(host(m(dev(x))), want)
        assert m.kernel_log == log, m.kernel_log
        np.testing.assert_array_equal(host(engine.LayerModel(net.spec)(dev(x))), want)


def test_a_captured_forward_replays_the_spatial_call():
    net = Z.SPECS["encdec_q4"][0]
    x = net.images()
    m = engine.GraphModel(net.spec)
    want = Z.reference(net.spec, x)
    pipe = engine.Pipelined(m, lanes=1, batch_size=2)
    xd = dev(np.concatenate([x, x[::-1]], axis=0))       # two full batches: captured, then replayed once
    got = host(pipe(xd))
    assert len(pipe._lanes) == 1 and all("graph" in ln for lanes in pipe._lanes.values() for ln in lanes)
    np.testing.assert_array_equal(got[:2], want)
    np.testing.assert_array_equal(got[2:], Z.reference(net.spec, x[::-1]))
    pipe.clear()
