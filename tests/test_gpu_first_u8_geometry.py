"""The default first layer at the benchmark's geometry: k_conv_first_u8_full (csrc/qnn_first_u8.hip, the un-pooled packed
byte kernel) at 224-wide images, short last row chunks and persistent grids that loop, on both of its entries, and the
"auto" first layer of BASELINE configs 4 and 5 end to end.

Every result is compared bit for bit with the uint8 specification (O.u8_conv_group / O.run_spec_u8) or with the exact
float32 path (O.run_spec(..., float_conv="device")); every test asserts the kernel it ran, so none passes on another
route.  Large batches compare three images with the oracle and the rest through batch independence."""
import zlib

import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine, nets
from oracle import qnn_oracle as O
from test_gpu_parity import BIN_ACT, Q, _oracle_group, _rand_bn, dev, host

pytestmark = pytest.mark.gpu
F32 = np.float32
BYTE_U8, BYTE_IMG = "mfma_i8_first_u8", "mfma_i8_first_img255"
EXACT_FIRST = ("mfma_f32_first", "mfma_f32_stem")          # the exact float32 first-layer kernels


def _full_grid(N, H, W, cout):
    """The launch of k_conv_first_u8_full as qnn_try_launch_first_u8 sizes it: tasks are (image, 16-column strip, chunk of
    rc row pairs); best_rc minimises rounds * (rc + 1.5) over even rc with six (cout 16) or three resident workgroups per
    CU; the grid has blocks_cap / slices workgroups of four waves per filter slice (blockIdx.y).  Returns rc, the chunks
    per strip, the row pairs of the last chunk, and how many times the persistent grid walks its task loop."""
    hp2, spr = H // 2, W // 16
    blocks_cap = 256 * (6 if cout == 16 else 3)
    best = None
    for rc in range(2, hp2 + 2, 2):
        nch = -(-hp2 // rc)
        cost = -(-(N * spr * nch) // (4 * blocks_cap)) * (rc + 1.5)
        if best is None or cost < best[0]:
            best = (cost, rc, nch)
    _, rc, nch = best
    ntasks = N * spr * nch
    slices = cout // (16 if cout == 16 else 64)
    waves = 4 * min(max(blocks_cap // slices, 1), -(-ntasks // 4))
    return dict(rc=rc, nch=nch, last=hp2 - (nch - 1) * rc, rounds=-(-ntasks // waves))


def _layer(name, cout, kind, nb):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    op = {"op": "conv", "kind": kind, "kernel": rng.uniform(-1, 1, (3, 3, 3, cout)).astype(F32),
          "strides": (1, 1), "padding": "same", "bias": (rng.standard_normal(cout) * 0.05).astype(F32)}
    if nb:
        op["nb"] = nb
    return rng, op, _rand_bn(rng, cout, 27 * 0.3)


class _Conv:
    """One first-layer group (conv + BN + activation, un-pooled, packed out) through qnn_conv2d_forward on either entry:
    uint8 images (QNN_STORE_U8) or float32 bytes / 255 with the image option (the default first layer's kernel)."""

    def __init__(self, op, bn, act, store):
        self.cout = op["kernel"].shape[3]
        self.w = engine._prepack(op, _abi.STORE_F32, torch.device("cuda"))
        self.inv, self.shift = (dev(a) for a in engine.bn_constants(bn))
        self.fn, ab = engine._act_code(act)
        self.ab = ab if self.fn == _abi.FN_QUANTIZED_TANH else 0
        self.nb = ab if ab else 1
        self.store = store

    def __call__(self, x):
        """-> (packed output (N*H*W, words), kernel name)."""
        N, H, W, _ = x.shape
        image = x.dtype == torch.float32
        if image:
            _abi.set_option("first_image", 1)
        try:
            y, _, _ = _abi.conv2d(self.w, x, _abi.STORE_U8 if not image else _abi.STORE_F32, 0, N, H, W, self.inv,
                                  self.shift, self.fn, self.ab, 1, self.store)
            kern = _abi.last_kernel()
        finally:
            if image:
                _abi.set_option("first_image", 0)
        return y, kern

    def values(self, y, N, H, W, pick=None):
        """Packed output -> float32 (N, H, W, cout) on the host (only the images in `pick`)."""
        v = _abi.unpack(y, N * H * W, self.cout, self.store, self.nb).reshape(N, H, W, self.cout)
        return host(v if pick is None else v[pick])


# name, cout, kind, nb, act, store, [(H, W, [N ...])]
#   stem 224 x 224: N = 1 -> rc = 2 (56 chunks of two row pairs each, 784 tasks, one round);
#                   N = 44 -> rc = 6, 19 chunks, the last one 4 row pairs, 11704 tasks on 6144 waves: two rounds.
#   stem 112 x 112: N = 512 -> rc = 12, 5 chunks, the last 8 row pairs, three rounds.
#   222 x 208 (111 row pairs, 13 strips): the last chunk is short for every rc; N = 48 (cout 16) -> rc = 6, two rounds;
#                   N = 24 (cout 64) -> rc = 6, two rounds; N = 16 (cout 192, three filter slices) -> rc = 8, three rounds.
#   VGG-large 32 x 32: N = 385 -> rc = 6, 3 chunks, the last 4 row pairs, four rounds;
#                     cout 64: N = 769 -> the same chunks, two rounds.
#   The int8 forms (16-byte stores) of the image entry wrote wrong first dwords at N = 64 and 385 before the wait state
#   behind their store (csrc/qnn_first_u8.hip); N <= 17 never showed it.
#   stem 10 x 16: the smallest seam -- five row pairs in tasks of 2, 2 and 1, one strip, one round.
FULL = [("stem_q4", 16, "quantized", 4, Q(4), _abi.STORE_I4,
         [(224, 224, [1, 44]), (112, 112, [1, 512]), (222, 208, [1, 48]), (10, 16, [2])]),
        ("stem_bin", 16, "binary", None, BIN_ACT, _abi.STORE_I4,
         [(224, 224, [1, 44]), (112, 112, [1, 512]), (222, 208, [1, 48])]),
        ("vgg_q8", 256, "quantized", 8, Q(8), _abi.STORE_I8, [(32, 32, [1, 385])]),
        ("c64_bin_i8", 64, "binary", None, BIN_ACT, _abi.STORE_I8, [(32, 32, [1, 769])]),
        ("c192_q4", 192, "quantized", 4, Q(4), _abi.STORE_I4, [(222, 208, [1, 16])]),
        ("c64_q4", 64, "quantized", 4, Q(4), _abi.STORE_I4, [(222, 208, [1, 24])])]
FULL_IDS = [c[0] for c in FULL]


def test_launch_mirror_reaches_the_edges_the_cases_name():
    """The batch sizes of FULL give what their comment says: the N = 1 runs take chunks of two row pairs; every larger N
    ends each image with a short chunk and walks the persistent grid more than once."""
    for name, cout, _, _, _, _, shapes in FULL:
        for H, W, Ns in shapes:
            g1 = _full_grid(1, H, W, cout)
            assert g1["rc"] == 2 and g1["rounds"] == 1, (name, H, W, g1)
            for N in Ns[1:]:
                g = _full_grid(N, H, W, cout)
                assert g["last"] < g["rc"] and g["rounds"] > 1, (name, H, W, N, g)


@pytest.mark.parametrize("case", FULL, ids=FULL_IDS)
def test_full_byte_kernel_at_benchmark_geometry(case):
    """k_conv_first_u8_full on uint8 images and on float32 bytes / 255: the specification bit for bit at 224 x 224
    (14 strips), 112 x 112, 222 x 208 (odd row-pair count, 13 strips) and 32 x 32, for N = 1 and an N that leaves a
    short last chunk in every image and loops the persistent grid.  Large N: the first, a middle and the last image
    against the oracle, every other image through a permuted batch (same rows, bit for bit)."""
    name, cout, kind, nb, act, store, shapes = case
    rng, op, bn = _layer("geom_" + name, cout, kind, nb)
    conv = _Conv(op, bn, act, store)
    for H, W, Ns in shapes:
        for N in Ns:
            xu8 = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
            pick = [0] if N == 1 else [0, N // 2, N - 1]
            want = O.u8_conv_group(xu8[pick], op, bn, act)
            xb, xf = dev(xu8), dev((xu8.astype(F32) / F32(255)).astype(F32))
            perm = torch.randperm(N, device="cuda") if N > 1 else None
            for xin, tag in ((xb, BYTE_U8), (xf, BYTE_IMG)):
                y, kern = conv(xin)
                assert kern == tag, (name, H, W, N, kern)
                np.testing.assert_array_equal(conv.values(y, N, H, W, pick), want, err_msg="%s %dx%d N=%d %s" % (name, H, W, N, tag))
                if perm is not None:
                    yp, kern = conv(xin[perm].contiguous())
                    assert kern == tag
                    assert torch.equal(yp.reshape(N, -1), y.reshape(N, -1)[perm]), (name, H, W, N, tag)
            conv.w.check()                              # bytes / 255 never raise the domain flag


@pytest.mark.parametrize("shape", [(2, 224, 218, 3), (2, 223, 224, 3)], ids=["w218", "h223"])
@pytest.mark.parametrize("case", [FULL[0], FULL[2]], ids=["stem_q4", "vgg_q8"])
def test_route_edges_next_to_the_full_byte_kernel(case, shape):
    """W % 16 != 0 and odd H are outside the byte kernel: the uint8 entry still equals its specification, and the image
    entry equals the exact float32 chain of the route it reports."""
    name, cout, kind, nb, act, store, _ = case
    rng, op, bn = _layer("edge_" + name, cout, kind, nb)
    conv = _Conv(op, bn, act, store)
    N, H, W, _ = shape
    xu8 = rng.integers(0, 256, shape, dtype=np.uint8)
    y, kern = conv(dev(xu8))
    assert kern not in (BYTE_U8, BYTE_IMG) and kern.startswith("generic_u8"), kern
    np.testing.assert_array_equal(conv.values(y, N, H, W), O.u8_conv_group(xu8, op, bn, act))
    x = (xu8.astype(F32) / F32(255)).astype(F32)
    y, kern = conv(dev(x))
    assert kern not in (BYTE_U8, BYTE_IMG) and (kern.startswith(EXACT_FIRST) or kern == "generic"), kern
    np.testing.assert_array_equal(conv.values(y, N, H, W), _oracle_group(x, op, bn, act, 1, float_conv="device"))


@pytest.mark.parametrize("cout", [16, 256])
def test_domain_flag_at_224_catches_one_off_grid_value(cout):
    """The image entry at 224 x 224, N = 4: a batch of bytes / 255 with 0.0 and 1.0 in it leaves the flag down; a single
    off-grid value raises it wherever it sits -- the last image's last pixel (channel 2), the last column of a strip
    (15) and the first of the next (16, read by the left strip as its halo too) in a middle row, row 0 of image 0."""
    name = "dom_%d" % cout
    case = FULL[0] if cout == 16 else FULL[2]
    rng, op, bn = _layer(name, cout, case[2], case[3])
    conv = _Conv(op, bn, case[4], case[5])
    N, H, W = 4, 224, 224
    xu8 = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    xu8[0, 5, 7, 1], xu8[3, 100, 200, 0] = 0, 255
    x = dev((xu8.astype(F32) / F32(255)).astype(F32))
    assert float(x.min()) == 0.0 and float(x.max()) == 1.0
    _, kern = conv(x)
    assert kern == BYTE_IMG
    conv.w.check()
    for at in ((N - 1, H - 1, W - 1, 2), (2, 117, 15, 0), (1, 117, 16, 1), (0, 0, 37, 2)):
        xb = x.clone()
        xb[at] = 0.123                                  # 31.365 / 255: off the byte grid
        _, kern = conv(xb)
        assert kern == BYTE_IMG
        with pytest.raises(_abi.QnnError, match="outside its domain"):
            conv.w.check()
    conv(x)
    conv.w.check()                                      # the check cleared the flag


# ---------------------------------------------------------------------------------------------------------------
# BASELINE configs 5 and 4 on the default ("auto") first layer
# ---------------------------------------------------------------------------------------------------------------
def _cfg5():
    cf = nets.baseline_config(4)
    assert (cf.nres, cf.dim, cf.wbits, cf.abits) == (10, 224, 4, 4)
    return cf, nets.build_spec(cf, nets.SEED_BASE + 4)[:-1]          # logits


def _no_exact_first(log):
    return not any(k.startswith(EXACT_FIRST) for k in log)


def test_config5_auto_first_layer_one_image():
    """ImageNet-224 ResNet, nres = 10, built with no first_layer argument: image floats take the byte kernel and give
    the uint8 specification (and the uint8 entry the same array); a Gaussian input gives the exact float32 path."""
    cf, spec = _cfg5()
    m = engine.ResidualFusedModel(spec)
    assert m.first_layer == "auto"
    xu8 = nets.synthetic_images_u8(cf, 1, 11)
    want = O.run_spec_u8(spec, xu8)
    m.kernel_log = []
    got = host(m(dev((xu8.astype(F32) / F32(255)).astype(F32))))
    assert m.kernel_log[0] == BYTE_IMG and _no_exact_first(m.kernel_log), m.kernel_log[:3]
    np.testing.assert_array_equal(got, want)
    m.check_domain()
    m.kernel_log = []
    np.testing.assert_array_equal(host(m(dev(xu8))), want)
    assert m.kernel_log[0] == BYTE_U8, m.kernel_log[:3]
    xf = np.random.default_rng(5).standard_normal(xu8.shape).astype(F32)
    np.testing.assert_array_equal(host(m(dev(xf))), O.run_spec(spec, xf, float_conv="device"))
    m.check_domain()


def test_config5_auto_first_layer_at_batch_64_and_pipelined():
    """Config 5 at its per-GPU batch on "auto": permuted and sliced batches give the same rows, image 0 equals the
    uint8 specification, the domain check passes; engine.Pipelined (2 lanes of 16, hipGraph replays) over 48 images
    equals the eager forward bit for bit."""
    cf, spec = _cfg5()
    m = engine.ResidualFusedModel(spec)
    N = 64
    xu8 = nets.synthetic_images_u8(cf, N, 12)
    x = dev((xu8.astype(F32) / F32(255)).astype(F32))
    m.kernel_log = []
    y = m(x)
    assert m.kernel_log[0] == BYTE_IMG and _no_exact_first(m.kernel_log), m.kernel_log[:3]
    perm = torch.randperm(N, device="cuda")
    assert torch.equal(m(x[perm].contiguous()), y[perm])
    assert torch.equal(m(x[37:41].contiguous()), y[37:41])
    np.testing.assert_array_equal(host(y[:1]), O.run_spec_u8(spec, xu8[:1]))
    m.check_domain()
    pipe = engine.Pipelined(m, lanes=2, batch_size=16)
    assert torch.equal(pipe(x[:48].contiguous()), y[:48])
    pipe.check_domain()


def test_config4_auto_first_layer_at_batch_4096():
    """VGG-large 8/8 (BASELINE config 4) at the benchmark's batch, FusedModel(spec) with no argument on bytes / 255:
    the byte kernel, the uint8 entry's bits, the specification on a slice spread over the batch, batch independence
    and a clean domain check."""
    cf = nets.baseline_config(3)
    spec = nets.build_spec(cf, nets.SEED_BASE + 3)
    m = engine.FusedModel(spec)
    assert m.first_layer == "auto"
    N = 4096
    xu8 = nets.synthetic_images_u8(cf, N, 4321)
    x = dev((xu8.astype(F32) / F32(255)).astype(F32))
    m.kernel_log = []
    y = m(x)
    assert m.kernel_log[0] == BYTE_IMG and _no_exact_first(m.kernel_log), m.kernel_log[:3]
    m.check_domain()
    m.kernel_log = []
    assert torch.equal(m(dev(xu8)), y)
    assert m.kernel_log[0] == BYTE_U8, m.kernel_log[:3]
    pick = np.arange(0, N, 97)
    np.testing.assert_array_equal(host(y[torch.as_tensor(pick, device="cuda")]), O.run_spec_u8(spec, xu8[pick]))
    perm = torch.randperm(N, device="cuda")
    assert torch.equal(m(x[perm].contiguous()), y[perm])
    assert torch.equal(m(x[1000:1037].contiguous()), y[1000:1037])
    m.check_domain()
