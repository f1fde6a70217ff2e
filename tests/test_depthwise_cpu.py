"""What the depthwise convolution promises that needs no GPU: the numpy reference of depthwise_cases.py against
torch.nn.functional.conv2d(groups=C) in float64 on every case geometry, the block-diagonal expansion identity, the 16-bit
bound with a constructed case that breaks a 16-bit lane, the layer classes' host surface, and the symbols of the header."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi

import depthwise_cases as D

ENTRIES = _abi.EXPORTS_DEPTHWISE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = sorted({(c["C"] if c["C"] < 10 else 3, c["M"], c["window"], c["stride"], c["same"], c["dil"], c["map"])
                     for c in D.geometry_cases()})


def torch_depthwise(x, w, stride, same, dil):
    """float64 grouped convolution of NHWC x with the Keras kernel (kh, kw, C, M), TensorFlow's padding made explicit."""
    N, H, W, C = x.shape
    kh, kw, _, M = w.shape
    Ho, pt = D.out_pad(H, kh, stride, same, dil[0])
    Wo, pl = D.out_pad(W, kw, stride, same, dil[1])
    pb = max((Ho - 1) * stride + dil[0] * (kh - 1) + 1 - H - pt, 0)
    pr = max((Wo - 1) * stride + dil[1] * (kw - 1) + 1 - W - pl, 0)
    xt = torch.nn.functional.pad(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), (pl, pr, pt, pb))
    wt = torch.from_numpy(w.astype(np.float64)).permute(2, 3, 0, 1).reshape(C * M, 1, kh, kw)
    y = torch.nn.functional.conv2d(xt, wt, stride=stride, dilation=dil, groups=C)
    return y.permute(0, 2, 3, 1).numpy()[:, :Ho, :Wo]


@pytest.mark.parametrize("C,M,window,stride,same,dil,shape", GEOMETRIES)
def test_reference_sum_equals_torch_grouped_conv(C, M, window, stride, same, dil, shape):
    rs = np.random.RandomState(11)
    x = rs.randint(-8, 8, shape + (C,))
    w = rs.randint(-8, 8, window + (C, M))
    got = D.dw_sum(x, w, stride, same, dil)
    want = torch_depthwise(x, w, stride, same, dil)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want.astype(np.int64))          # integers: float64 is exact here
    xf = rs.randn(*x.shape).astype(np.float32)
    wf = rs.randn(*w.shape).astype(np.float32)
    np.testing.assert_allclose(D.dw_sum(xf, wf, stride, same, dil, np.float64), torch_depthwise(xf, wf, stride, same, dil),
                               rtol=0, atol=1e-12 * window[0] * window[1] * 16)


@pytest.mark.parametrize("M,stride,same", [(1, 1, True), (2, 2, False), (3, 1, False)])
def test_block_diagonal_expansion_identity(M, stride, same):
    rs = np.random.RandomState(12)
    C = 5
    x = rs.randint(-8, 8, (2, 5, 7, C))
    k = rs.randint(-8, 8, (3, 3, C, M))
    full = D.expand_block_diagonal(k)
    assert full.shape == (3, 3, C, C * M) and np.count_nonzero(full) == np.count_nonzero(k)
    Ho, pt = D.out_pad(5, 3, stride, same)
    Wo, pl = D.out_pad(7, 3, stride, same)
    want = np.zeros((2, Ho, Wo, C * M), np.int64)
    xp = np.zeros((2, 5 + 4, 7 + 4, C), np.int64)
    xp[:, 2:7, 2:9] = x
    for oy in range(Ho):
        for ox in range(Wo):
            patch = xp[:, oy * stride - pt + 2:oy * stride - pt + 5, ox * stride - pl + 2:ox * stride - pl + 5]
            want[:, oy, ox] = np.einsum("nyxc,yxco->no", patch, full)
    np.testing.assert_array_equal(D.dw_sum(x, k, stride, same), want)
    # quantize(0) = 0 keeps the expansion exact; binarize(0) is not 0, and the ternary cutoff is a mean over the kernel
    assert D.quantize_weights(np.zeros(4, np.float32), D.W_QUANT, 4)[1].tolist() == [0, 0, 0, 0]
    assert D.quantize_weights(np.zeros(4, np.float32), D.W_BINARY)[1].tolist() == [-1, -1, -1, -1]
    kt = (rs.randint(-64, 65, (3, 3, C, 1)) / 64.0).astype(np.float32)
    assert not np.array_equal(D.expand_block_diagonal(D.quantize_weights(kt, D.W_TERNARY)[0]),
                              D.quantize_weights(D.expand_block_diagonal(kt), D.W_TERNARY)[0])


def test_the_16_bit_bound():
    assert D.pk16_bound_ok(3, 3, 4, 3) and 9 * 8 * 8 == 576
    assert not D.pk16_bound_ok(3, 3, 8, 7) and 9 * 128 * 128 == 147456
    assert D.pk16_bound_ok(3, 3, 6, 6) and not D.pk16_bound_ok(3, 3, 7, 6)          # 18432 < 2^15 <= 36864
    assert [D.takes_pk16(c) for c in D.bound_cases()] == [True, True, True, False, True, False]
    assert not D.takes_pk16(D._case(D.I4, 8, stride=2)) and not D.takes_pk16(D._case(D.I4, 8, M=2))
    c, x, kernel = D.overflow_case()
    codes = D.quantize_weights(kernel, c["wkind"], c["wbits"])[1]
    assert codes.min() == codes.max() == -128
    acc = D.dw_sum(x, codes, 1, True)
    assert acc.max() == 147456 > 2 ** 15 - 1
    assert 2 * 128 * 128 > 2 ** 15 - 1                                              # the second tap's partial sum already
    wrapped = ((acc + 2 ** 15) % 2 ** 16) - 2 ** 15                                 # what a 16-bit lane would hold
    assert not np.array_equal(wrapped, acc)
    want = D.reference(c, x, kernel, None, None)
    assert want.max() == np.float32(9.0) and want.min() == np.float32(4.0)          # interior 9 taps, corners 4


def test_encode_decode_round_trip():
    rs = np.random.RandomState(13)
    for store, bits, C in ((D.BIN, 1, 33), (D.I4, 4, 9), (D.I4, 2, 8), (D.I8, 8, 5)):
        codes = D.random_codes(rs, (3, C), store, bits)
        back, spare = D.decode(D.encode(codes, store), store, C)
        np.testing.assert_array_equal(back, codes)
        assert not spare.any()
        dirty = D.encode(codes, store, spare=rs)
        np.testing.assert_array_equal(D.decode(dirty, store, C)[0], codes)
    t = D.random_codes(rs, (3, 33), D.T2, 1)
    w = D.encode(t, D.T2)
    assert w.shape == (3, 4)
    mask = (w[:, 0::2, None] >> np.arange(32, dtype=np.uint32)) & 1
    sign = (w[:, 1::2, None] >> np.arange(32, dtype=np.uint32)) & 1
    np.testing.assert_array_equal((mask * (2 * sign.astype(np.int64) - 1)).reshape(3, -1)[:, :33], t)


# ---- the multitask table: what it reaches, and that its expected values can tell pixel mappings apart ------------------------
FILL = 0x5A5A5A5A                                # what test_gpu_depthwise.py lays under every output


def test_multitask_table_reaches_the_decodes_it_names():
    cases = D.multitask_cases()
    assert len({D.case_id(c) for c in cases}) == len(cases) == 9 and all(c["map"][0] >= 2 for c in cases)
    fast = [c for c in cases if D.takes_pk16(c)]
    assert len(fast) == 7 and {(c["store"], c["C"]) for c in fast} == {(D.I4, 33), (D.I8, 16)}
    # row blocks, rows of the last block and items, restated from the map alone ('same' at stride 1: Ho = H, Wo = W)
    by_map = {(3, 10, 9): (3, 2, {D.I4: 405, D.I8: 324}), (2, 8, 17): (2, 4, {D.I4: 340, D.I8: 272}),
              (2, 13, 5): (4, 1, {D.I4: 200, D.I8: 160}), (70, 1, 1): (1, 1, {D.I4: 350})}
    for c in fast:
        N, H, W = c["map"]
        blocks, last, items = D.pk16_items(c)
        assert (blocks, last, items) == (-(-H // 4), (H - 1) % 4 + 1, N * -(-H // 4) * W * -(-c["C"] // (32 // c["store"])))
        assert (blocks, last, items) == by_map[c["map"]][:2] + (by_map[c["map"]][2][c["store"]],), D.case_id(c)
    for store in (D.I4, D.I8):
        mine = [D.pk16_items(c) for c in fast if c["store"] == store]
        # past the first workgroup with a second, partly filled one; every raggedness of the last row block but 3
        assert any(items > D.BLOCK and items % D.BLOCK for _, _, items in mine)
        assert {last % D.K_ROWS for blocks, last, items in mine if items > D.BLOCK or blocks > 2} >= {0, 1, 2}
        assert max(blocks for blocks, _, _ in mine) >= 3
    assert any(items > D.BLOCK and last % D.K_ROWS in (0, 1, 2) for _, last, items in map(D.pk16_items, fast))
    assert any(c["map"] == D.TINY_MAP and D.pk16_items(c)[2] == 350 for c in fast)
    # the plain form past one workgroup at V = 4, and the same case at V = 1
    plain = [c for c in cases if not D.takes_pk16(c)]
    assert [c["misalign"] for c in plain] == [False, True] and all((c["store"], c["C"]) == (D.BIN, 256) for c in plain)
    items = [D.plain_items(c["out_store"], c["C"], 2 * 9 * 9, c["misalign"]) for c in plain]
    assert items == [(4, 324), (1, 1296)] and items[0][1] > D.BLOCK and items[0][1] % D.BLOCK


@pytest.mark.parametrize("c", D.multitask_cases(), ids=D.case_id)
def test_multitask_expected_values_tell_pixel_mappings_apart(c):
    """At most half of the codes at the clip ends (the 1-bit store: each code at least a quarter), no two images, no two
    16-pixel runs and no two row blocks of an image alike, and no expected word equal to the pattern the GPU test lays
    under the output."""
    want = D.reference(c, *D.make_inputs(c, c["seed"]))
    assert D.degenerate(c, want) == []
    blocks = [[img[r:r + D.K_ROWS].reshape(-1, img.shape[-1]) for r in range(0, img.shape[0], D.K_ROWS)] for img in want]
    assert D.degenerate(c, want, blocks) == []
    assert not (D.encode(want, c["out_store"]) == FILL).any()
    if D.takes_pk16(c):                          # the GPU test writes the same codes to the other packed store as well
        assert c["act_bits"] == 4 and not (D.encode(want, D.I4 + D.I8 - c["out_store"]) == FILL).any()


LAYERS = [(qnn_amd.DepthwiseConv2D, {}), (qnn_amd.BinaryDepthwiseConv2D, {"H": 1.0}),
          (qnn_amd.QuantizedDepthwiseConv2D, {"nb": 4}), (qnn_amd.TernaryDepthwiseConv2D, {})]


@pytest.mark.parametrize("cls,kw", LAYERS)
def test_layer_host_surface(cls, kw):
    layer = cls((3, 2), strides=2, padding="same", depth_multiplier=2, use_bias=False, device="cpu", name="dw", **kw)
    cfg = layer.get_config()
    assert cfg["kernel_size"] == (3, 2) and cfg["depth_multiplier"] == 2 and cfg["strides"] == (2, 2)
    assert cfg["padding"] == "same" and cfg["dilation_rate"] == (1, 1) and cfg["use_bias"] is False
    if "nb" in kw:
        assert cfg["nb"] == 4
    again = cls.from_config(dict(cfg, device="cpu"))
    assert again.get_config() == cfg
    assert layer.compute_output_shape((None, 9, 7, 5)) == (None, 5, 4, 10)
    valid = cls(3, dilation_rate=2, device="cpu")
    assert valid.compute_output_shape((4, 9, 7, 5)) == (4, 5, 3, 5)
    layer.build((None, 9, 7, 5))
    assert tuple(layer.kernel.shape) == (3, 2, 5, 2) and layer.bias is None and layer.count_params() == 60
    assert [w.shape for w in layer.get_weights()] == [(3, 2, 5, 2)]
    with pytest.raises(ValueError):
        layer.set_weights([np.zeros((3, 2, 5, 1), np.float32)])
    with pytest.raises(ValueError):
        layer.set_weights([np.zeros((3, 2, 5, 2), np.float32), np.zeros(10, np.float32)])
    layer.set_weights([np.ones((3, 2, 5, 2), np.float32)])
    for bad in ({"strides": 2, "dilation_rate": 2}, {"padding": "full"}, {"depth_multiplier": 0}):
        with pytest.raises(ValueError):
            cls(3, device="cpu", **bad)
    for bad in ({"data_format": "channels_first"}, {"strides": (1, 2)}, {"strides": 3}):
        with pytest.raises(_abi.QnnError):
            cls(3, device="cpu", **bad)
    with pytest.raises(_abi.QnnError):
        cls(8, device="cpu")
    with pytest.raises(TypeError):
        cls(3, device="cpu", filters=4)
    with pytest.raises(_abi.QnnError):                       # no CPU path
        layer(torch.zeros(1, 9, 7, 5))


def test_header_declares_what_the_library_exports():
    text = open(os.path.join(ROOT, "include", "qnn_abi_depthwise.h")).read()
    declared = set(re.findall(r"^int\s+(qnn_\w+)\(", text, re.M))
    assert declared == set(ENTRIES)
    build = importlib.import_module("quantizedneuralnetworks-keras-tensorflow_amd._build")
    assert "qnn_depthwise.hip" in build.SOURCES
    assert any(h.endswith("qnn_abi_depthwise.h") for h in build._headers())
    abi_h = open(os.path.join(ROOT, "include", "qnn_abi.h")).read()
    assert "#define QNN_ABI_VERSION 4" in abi_h and "depthwise" not in abi_h
    if not os.path.exists(build.LIB) or build.needs_build():
        pytest.skip("the in-tree library is not built")
    lib = _abi.load()                                         # raises if a declared symbol is not exported
    for name in ENTRIES:
        assert getattr(lib, name) is not None
    assert lib.qnn_version() == 4


def _npz(tmp_path, layers, arrays):
    import json
    cfg = {"class_name": "Model", "config": {"layers": layers}}
    path = str(tmp_path / "net.npz")
    np.savez(path, model_config_json=np.frombuffer(json.dumps(cfg).encode(), np.uint8), **arrays)
    return path


def _layer(cls, name, src, **config):
    return {"class_name": cls, "name": name, "config": dict(config, name=name), "inbound_nodes": [[[src, 0, 0, {}]]] if src else []}


def test_importer_maps_depthwise_and_separable(tmp_path):
    from qnn_amd import nets
    rs = np.random.RandomState(21)
    arrays = {"dw/depthwise_kernel": rs.randn(3, 3, 4, 2).astype(np.float32), "dw/bias": rs.randn(8).astype(np.float32),
              "sep/depthwise_kernel": rs.randn(5, 5, 8, 1).astype(np.float32),
              "sep/pointwise_kernel": rs.randn(1, 1, 8, 6).astype(np.float32), "sep/bias": rs.randn(6).astype(np.float32)}
    common = dict(padding="same", data_format="channels_last", activation="linear", use_bias=True)
    layers = [_layer("InputLayer", "in", None),
              _layer("DepthwiseConv2D", "dw", "in", kernel_size=[3, 3], strides=[2, 2], depth_multiplier=2,
                     dilation_rate=[1, 1], **common),
              _layer("SeparableConv2D", "sep", "dw", kernel_size=[5, 5], strides=[1, 1], depth_multiplier=1, filters=6,
                     dilation_rate=[2, 2], **common)]
    spec = nets.spec_from_keras_npz(_npz(tmp_path, layers, arrays))
    assert [op["op"] for op in spec] == ["dwconv", "dwconv", "conv"]
    dw, sdw, pw = spec
    assert dw["kind"] == "float" and dw["src"] == "input" and dw["dst"] == "dw" and dw["depth_multiplier"] == 2
    assert dw["strides"] == (2, 2) and dw["padding"] == "same" and dw["dilation"] == (1, 1)
    np.testing.assert_array_equal(dw["kernel"], arrays["dw/depthwise_kernel"])
    np.testing.assert_array_equal(dw["bias"], arrays["dw/bias"])
    assert sdw["bias"] is None and sdw["src"] == "dw" and sdw["dst"] == "sep_depthwise" and sdw["dilation"] == (2, 2)
    np.testing.assert_array_equal(sdw["kernel"], arrays["sep/depthwise_kernel"])
    assert pw["kind"] == "float" and pw["src"] == "sep_depthwise" and pw["dst"] == "sep" and pw["strides"] == (1, 1)
    assert "dilation_rate" not in pw
    np.testing.assert_array_equal(pw["kernel"], arrays["sep/pointwise_kernel"])
    np.testing.assert_array_equal(pw["bias"], arrays["sep/bias"])
    for cls in ("DepthwiseConv2D", "SeparableConv2D"):
        name = "dw" if cls == "DepthwiseConv2D" else "sep"
        bad = [layers[0], _layer(cls, name, "in", kernel_size=[3, 3], strides=[1, 1], depth_multiplier=1, dilation_rate=[1, 1],
                                 **dict(common, data_format="channels_first"))]
        with pytest.raises(ValueError, match="channels_first"):
            nets.spec_from_keras_npz(_npz(tmp_path, bad, arrays))


def test_fused_engines_decline_and_epilogue_cases_hold_ties_and_clips():
    from qnn_amd import engine
    spec = [{"op": "dwconv", "kind": "quantized", "nb": 4, "kernel": np.zeros((3, 3, 8, 1), np.float32), "bias": None,
             "strides": (1, 1), "padding": "same", "dilation": (1, 1), "depth_multiplier": 1, "H": 1.0}]
    for cls in (engine.FusedModel, engine.ResidualFusedModel):
        with pytest.raises(_abi.NotFusable, match="dwconv"):
            cls(spec, "cpu")
    # every quantised-activation epilogue case on packed input holds a clipped value, and an exact rounding tie where the
    # activation grid is coarser than the pre-activations' step
    seen = 0
    for c in D.epilogue_cases():
        if c["fn"] not in D.QACTS or c["store"] == D.F32:
            continue
        x, kernel, bias, bn = D.make_inputs(c)
        pre = D.reference(dict(c, fn=D.FN_NONE, act_bits=0, out_store=D.F32), x, kernel, bias, bn).astype(np.float64)
        m = 2.0 ** (c["act_bits"] - 1)
        if c["fn"] == D.FN_QUANTIZED_RELU:
            t, lo = (pre + 1) * m - m, 0
        else:
            t, lo = pre * m, -m
        # (a wider grid is finer than the pre-activations' own steps; 8-bit x 8-bit sums step by 2^-14, where a tie is chance)
        # and +-1 / ternary codes without bias and BN sum to whole numbers)
        if c["act_bits"] <= 4 and c["store"] == D.I4:
            assert (t - np.floor(t) == 0.5).any(), D.case_id(c)
        assert (t > m - 1).any() or (t < lo).any(), D.case_id(c)      # a value beyond the grid: it is clipped
        seen += 1
    assert seen > 100
    # one tie and one clipped value are a low bar for random inputs.  The counted points -- at least 32 ties strictly inside
    # the clip range and 8 points on each clip edge, per kernel form, activation, width and BN sign -- are conditions of the
    # cases of sideconv_grid_cases.py; test_sideconv_grid_cpu.py asserts them on every case and says what is exempt.  Here
    # only that those cases exist for every depthwise form, and the counts on the one this test used to speak of
    import sideconv_grid_cases as S
    grid = [c for c in S.cases() if c["op"] == "dw" and c["fn"] in D.QACTS and S.claims(c, c["act_bits"])]
    assert len(grid) > 300 and {c["form"] for c in grid} == {"depthwise_" + s for s in ("i4", "i8", "i4_plain", "i8_plain", "bin", "t2", "f32")}
    for c in (k for k in grid if k["form"] == "depthwise_i4" and k["act_bits"] == 4):
        n = S.counts(c, S.preactivation(c))
        assert n["ties"] >= S.MIN_TIES and n["hi"] >= S.MIN_EDGE and n["beyond"] >= S.MIN_EDGE, (c["id"], n)
