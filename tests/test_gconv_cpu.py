"""The grouped convolution without a GPU: the numpy reference of gconv_cases.py against torch's conv2d(groups=g) in float64
on every case geometry, against the block-diagonal expansion and, at groups == Cin, against the depthwise reference; the
route rule on its boundary table; the layer classes' host surface; the importer on hand-built .npz files; the exported
symbols and their ctypes prototypes."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import qnn_amd                                   # noqa: F401  (the package alias of conftest.py)
from qnn_amd import _abi, engine, nets

import depthwise_cases as D
import gconv_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = _abi.EXPORTS_GCONV                     # read at import: without the feature nothing below means anything


def _geometries():
    seen, out = set(), []
    for c in G.plain_cases() + G.mfma_cases() + G.boundary_cases() + G.multitask_cases():
        key = (c["Cg"], c["Fg"], c["groups"], c["window"], c["stride"], c["same"], c["dil"], c["map"])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def _torch_conv(x, w, groups, stride, same, dil):
    """torch.nn.functional.conv2d in float64 with TensorFlow's padding laid on explicitly."""
    N, H, W, _ = x.shape
    kh, kw = w.shape[:2]
    Ho, pt = G.out_pad(H, kh, stride, same, dil[0])
    Wo, pl = G.out_pad(W, kw, stride, same, dil[1])
    if Ho <= 0 or Wo <= 0:
        return np.zeros((N, max(Ho, 0), max(Wo, 0), w.shape[3]))
    pb = max((Ho - 1) * stride + dil[0] * (kh - 1) + 1 - H - pt, 0)
    pr = max((Wo - 1) * stride + dil[1] * (kw - 1) + 1 - W - pl, 0)
    xt = torch.nn.functional.pad(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), (pl, pr, pt, pb))
    wt = torch.from_numpy(w.astype(np.float64)).permute(3, 2, 0, 1).contiguous()          # (Cout, Cg, kh, kw)
    y = torch.nn.functional.conv2d(xt, wt, None, stride, 0, dil, groups)
    return y.permute(0, 2, 3, 1).numpy()[:, :Ho, :Wo]


def test_reference_equals_torch_conv2d_groups_and_the_block_diagonal_expansion():
    rs = np.random.RandomState(11)
    for c in _geometries():
        N, H, W = c["map"]
        kh, kw = c["window"]
        x = rs.randint(-8, 8, (N, H, W, c["Cin"]))
        w = rs.randint(-8, 8, (kh, kw, c["Cg"], c["Cout"]))
        got = G.gconv_sum(x, w, c["groups"], c["stride"], c["same"], c["dil"])
        want = _torch_conv(x, w, c["groups"], c["stride"], c["same"], c["dil"])
        assert got.shape == want.shape, G.case_id(c)
        np.testing.assert_array_equal(got, want, err_msg=G.case_id(c))
        full = G.gconv_sum(x, G.expand_block_diagonal(w, c["groups"]), 1, c["stride"], c["same"], c["dil"])
        np.testing.assert_array_equal(got, full, err_msg=G.case_id(c))


@pytest.mark.parametrize("C,M", [(5, 1), (4, 2), (3, 3)])
def test_groups_equal_channels_is_the_depthwise_reference(C, M):
    rs = np.random.RandomState(12)
    x = rs.randint(-8, 8, (2, 5, 6, C))
    w = rs.randint(-8, 8, (3, 3, C, M))
    for stride, same, dil in ((1, True, (1, 1)), (2, False, (1, 1)), (1, True, (2, 1))):
        np.testing.assert_array_equal(G.gconv_sum(x, w.reshape(3, 3, 1, C * M), C, stride, same, dil),
                                      D.dw_sum(x, w, stride, same, dil))


def test_ternary_cutoff_runs_over_the_grouped_kernel_not_the_expansion():
    k = (np.random.RandomState(3).randint(-64, 65, (3, 3, 2, 8)) / 64.0).astype(np.float32)
    q = G.quantize_weights(k, G.W_TERNARY)[0]
    qe = G.quantize_weights(G.expand_block_diagonal(k, 4), G.W_TERNARY)[0]
    assert not np.array_equal(G.expand_block_diagonal(q, 4), qe)       # the structural zeros lower the expansion's mean


def test_route_rule_on_its_boundary_table():
    for (kh, kw, cin, cout, g), want in G.ROUTE_TABLE:
        assert (G.plan(kh, kw, cin, cout, g) is not None) == want, (kh, kw, cin, cout, g)
        Cg, Fg = cin // g, cout // g
        for store in (G.I4, G.I8):
            assert G.takes_mfma(G._case(store, Cg, Fg, g, window=(kh, kw))) == want
            assert not G.takes_mfma(G._case(store, Cg, Fg, g, window=(kh, kw), out_store=G.F32))
            assert not G.takes_mfma(G._case(store, Cg, Fg, g, window=(kh, kw), misalign=True))
        assert not G.takes_mfma(G._case(G.BIN, Cg, Fg, g, window=(kh, kw)))
        assert not G.takes_mfma(G._case(G.I4, Cg, Fg, g, window=(kh, kw), out_store=G.I8))
    assert all(G.takes_mfma(c) for c in G.mfma_cases()) and not any(G.takes_mfma(c) for c in G.boundary_cases())
    assert not any(G.takes_mfma(c) for c in G.plain_cases() + G.weight_cases() + G.epilogue_cases())
    # ResNeXt-50 32x4d: R = 16, 16, 16, 32 and 3, 3, 3, 5 MFMAs per tile
    assert [(G.plan(3, 3, c, c, 32)["R"], G.plan(3, 3, c, c, 32)["steps"]) for c in (128, 256, 512, 1024)] == \
        [(16, 3), (16, 3), (16, 3), (32, 5)]
    shapes = {(c["Cg"], c["Fg"], c["groups"]) for c in G.mfma_cases()}
    assert shapes == set(G.MFMA_SHAPES)
    assert G.int32_refused(7, 7, 4096, 8, 7) and not G.int32_refused(7, 7, 4096, 7, 7)
    assert 7 * 7 * G.MAX_RUN * 8 * 8 * 16 < (1 << 31)        # the code * 16 int4 operands of the matrix-pipe form fit too


# ---- the multitask table: what it reaches, and that its expected values can tell pixel mappings apart ------------------------
FILL = 0x5A5A5A5A                                # what test_gpu_gconv.py lays under every output


def test_multitask_table_reaches_the_decodes_it_names():
    cases = G.multitask_cases()
    assert len({G.case_id(c) for c in cases}) == len(cases) == 27 and all(c["map"][0] >= 2 for c in cases)
    fast = [c for c in cases if G.takes_mfma(c)]
    assert len(fast) == 25 and {c["store"] for c in fast} == {G.I4, G.I8}
    assert {(c["Cg"], c["Fg"], c["groups"]) for c in fast} == set(G.MULTITASK_SHAPES) <= set(G.MFMA_SHAPES)
    assert {G.plan(3, 3, c["Cin"], c["Cout"], c["groups"])["t"] for c in fast} == {1, 4, 16}
    # the task count, restated from the map alone: GT = ceil(ceil(Ho * Wo / 16) / 4), waves = N * GT * tiles
    by_map = {(2, 9, 9): (81, 2), (2, 5, 29): (145, 3), (3, 17, 9): (32, 1), (2, 19, 15): (80, 2), (70, 1, 1): (1, 1)}
    for c in fast:
        N, H, W = c["map"]
        Ho, Wo = (G.out_pad(v, 3, c["stride"], c["same"])[0] for v in (H, W))
        npix, groups, GT, waves = G.wave_tasks(c)
        assert (npix, GT) == (Ho * Wo, -(-(-(-Ho * Wo // 16)) // 4)) == by_map[c["map"]], G.case_id(c)
        assert waves == N * GT * c["Cout"] // 16
    tasks = [G.wave_tasks(c) for c in fast]
    assert max(t[2] for t in tasks) >= 3                                  # g0 = 8
    i4 = [G.wave_tasks(c) for c in fast if c["store"] == G.I4]
    # int4 pairs (2 k, 2 k + 1) of a later task: a last group with an even index has no partner at all ...
    assert any((groups - 1) % 2 == 0 and groups - 1 >= G.K_PG for _, groups, _, _ in i4)
    # ... and a ragged last group with an odd index leaves 15 lanes of the pair with one valid member
    assert any((groups - 1) % 2 == 1 and groups - 1 >= G.K_PG and npix % 16 == 1 for npix, groups, _, _ in i4)
    # a later task that ends in two groups beyond the image
    assert any(GT * G.K_PG - groups >= 2 and GT >= 2 for _, groups, GT, _ in tasks)
    # the wave >= waves exit inside a partly filled workgroup, behind several tasks per image, and on the tiny images
    assert any(waves % (D.BLOCK // 64) and GT >= 2 for _, _, GT, waves in tasks)
    assert any(c["map"] == D.TINY_MAP and G.wave_tasks(c)[3] == 70 for c in fast)
    # the plain form past one workgroup at V = 4, and the same case at V = 1
    plain = [c for c in cases if not G.takes_mfma(c)]
    assert [c["misalign"] for c in plain] == [False, True] and all(c["store"] == G.I4 for c in plain)
    assert G.plan(3, 3, plain[0]["Cin"], plain[0]["Cout"], plain[0]["groups"]) is not None and plain[0]["out_store"] == G.F32
    items = [D.plain_items(c["out_store"], c["Cout"], 2 * 9 * 11, c["misalign"]) for c in plain]
    assert items == [(4, 1584), (1, 6336)] and items[0][1] > D.BLOCK and items[0][1] % D.BLOCK


@pytest.mark.parametrize("c", G.multitask_cases(), ids=G.case_id)
def test_multitask_expected_values_tell_pixel_mappings_apart(c):
    """At most half of the codes at the clip ends, no two images and no two 16-pixel groups of an image alike, and no
    expected word equal to the pattern the GPU test lays under the output."""
    want = G.reference(c, *G.make_inputs(c, c["seed"]))
    assert D.degenerate(c, want) == []
    words = want.view(np.uint32) if c["out_store"] == G.F32 else G.encode(want, c["out_store"])
    assert not (words == FILL).any()


# ---- the layer classes' host surface ------------------------------------------------------------------------------------------
CLASSES = (qnn_amd.GroupedConv2D, qnn_amd.BinaryGroupedConv2D, qnn_amd.QuantizedGroupedConv2D, qnn_amd.TernaryGroupedConv2D)


def test_layer_classes_host_surface():
    for cls in CLASSES:
        for kw in (dict(data_format="channels_first"), dict(strides=3), dict(strides=(1, 2)), dict(kernel_size=(8, 1))):
            with pytest.raises(_abi.QnnError):
                cls(**dict(dict(filters=8, kernel_size=3), **kw))
        with pytest.raises(ValueError, match="dilation_rate"):
            cls(8, 3, strides=2, dilation_rate=2)
        with pytest.raises(ValueError, match="groups"):
            cls(8, 3, groups=0)
        with pytest.raises(ValueError, match="padding"):
            cls(8, 3, padding="full")
        with pytest.raises(TypeError):
            cls(8, 3, depth_multiplier=2)
        with pytest.raises(ValueError, match="number of filters must be evenly divisible by the number of groups"):
            cls(8, 3, groups=3, device="cpu").build((None, 5, 5, 9))
        with pytest.raises(ValueError, match="number of input channels must be evenly divisible by the number of groups"):
            cls(9, 3, groups=3, device="cpu").build((None, 5, 5, 8))
        layer = cls(12, (3, 5), groups=4, strides=2, padding="same", device="cpu", seed=1)
        layer.build((None, 9, 9, 8))
        assert tuple(layer.kernel.shape) == (3, 5, 2, 12) and tuple(layer.bias.shape) == (12,)
        assert layer.compute_output_shape((2, 9, 10, 8)) == (2, 5, 5, 12)
        assert cls(4, 3, dilation_rate=(2, 3)).compute_output_shape((1, 9, 9, 4)) == (1, 5, 3, 4)
        cfg = layer.get_config()
        assert cfg["groups"] == 4 and cfg["filters"] == 12 and cfg["kernel_size"] == (3, 5) and cfg["strides"] == (2, 2)
        again = cls.from_config(dict(cfg, device="cpu"))
        assert again.get_config() == cfg
    q = qnn_amd.QuantizedGroupedConv2D(12, 3, groups=4, nb=4, H="Glorot", device="cpu")
    q.build((None, 5, 5, 8))
    # 'Glorot' on one group's fans: Cg * kh * kw = 18 in, Fg * kh * kw = 27 out
    assert q.H == np.float32(np.sqrt(1.5 / (18 + 27))) and q.kernel_lr_multiplier == np.float32(1.0 / np.sqrt(1.5 / (18 + 27)))
    assert q.get_config()["nb"] == 4
    assert "nb" not in qnn_amd.GroupedConv2D(4, 3).get_config()


def test_fused_engines_decline_and_model_picks_graphmodel_rule():
    spec = [{"op": "gconv", "kind": "quantized", "nb": 4, "kernel": np.zeros((3, 3, 4, 16), np.float32), "bias": None,
             "groups": 4, "strides": (1, 1), "padding": "same", "dilation": (1, 1), "H": 1.0}]
    for cls in (engine.FusedModel, engine.ResidualFusedModel):
        with pytest.raises(_abi.NotFusable, match="gconv.*GraphModel"):
            cls(spec, "cpu")
    assert engine._dilation(dict(spec[0], dilation=(2, 3))) == (2, 3)


# ---- the importer ----------------------------------------------------------------------------------------------------------
def _npz(tmp_path, layers, arrays):
    cfg = {"class_name": "Model", "config": {"layers": layers}}
    path = str(tmp_path / "net.npz")
    np.savez(path, model_config_json=np.frombuffer(json.dumps(cfg).encode(), np.uint8), **arrays)
    return path


def _layer(cls, name, src, **config):
    return {"class_name": cls, "name": name, "config": dict(config, name=name), "inbound_nodes": [[[src, 0, 0, {}]]] if src else []}


COMMON = dict(padding="same", data_format="channels_last", activation="linear", use_bias=True, dilation_rate=[1, 1],
              kernel_size=[3, 3], strides=[1, 1])


def test_importer_maps_grouped_layers_to_gconv(tmp_path):
    rs = np.random.RandomState(2)
    names = [("Conv2D", "g0", "float", 2, {}), ("QuantizedConv2D", "g1", "quantized", 4, {"H": 1.0, "kernel_lr_multiplier": 2.5}),
             ("BinaryConv2D", "g2", "binary", 2, {"H": 1.0}), ("TernaryConv2D", "g3", "ternary", 2, {"H": 0.5}),
             ("GroupedConv2D", "g4", "float", 1, {}), ("BinaryGroupedConv2D", "g5", "binary", 4, {"H": 1.0}),
             ("QuantizedGroupedConv2D", "g6", "quantized", 2, {"H": 1.0, "nb": 8}),
             ("TernaryGroupedConv2D", "g7", "ternary", 8, {"H": 1.0})]
    arrays, layers, src = {}, [_layer("InputLayer", "in", None)], "in"
    for cls, name, kind, g, extra in names:
        arrays[name + "/kernel"] = rs.rand(3, 3, 8 // g, 8).astype(np.float32)
        arrays[name + "/bias"] = rs.rand(8).astype(np.float32)
        layers.append(_layer(cls, name, src, filters=8, groups=g, **dict(COMMON, **extra)))
        src = name
    spec = nets.spec_from_keras_npz(_npz(tmp_path, layers, arrays), wbits=4, abits=4)
    assert [op["op"] for op in spec] == ["gconv"] * 8
    assert [op["kind"] for op in spec] == [n[2] for n in names] and [op["groups"] for op in spec] == [n[3] for n in names]
    assert spec[0]["src"] == "input" and spec[1]["src"] == "g0" and [op["dst"] for op in spec] == [n[1] for n in names]
    assert spec[1]["nb"] == 4 and spec[6]["nb"] == 8 and spec[3]["H"] == 0.5 and spec[1]["klm"] == np.float32(2.5)
    for op, (_, name, _, _, _) in zip(spec, names):
        assert op["strides"] == (1, 1) and op["padding"] == "same" and op["dilation"] == (1, 1)
        np.testing.assert_array_equal(op["kernel"], arrays[name + "/kernel"])
        np.testing.assert_array_equal(op["bias"], arrays[name + "/bias"])
    dil = [layers[0], _layer("Conv2D", "g0", "in", filters=8, groups=2, **dict(COMMON, dilation_rate=[2, 3], use_bias=False))]
    op = nets.spec_from_keras_npz(_npz(tmp_path, dil, arrays))[0]
    assert op["op"] == "gconv" and op["dilation"] == (2, 3) and op["bias"] is None
    for cls, name, _, g, extra in names:
        for change, match in ((dict(activation="relu"), "activation"), (dict(data_format="channels_first"), "channels_first"),
                              (dict(groups=3), "groups")):
            if change.get("groups") and g == 1:
                continue
            bad = [layers[0], _layer(cls, name, "in", filters=8, **dict(dict(COMMON, groups=g, **extra), **change))]
            with pytest.raises(ValueError, match=match) as err:
                nets.spec_from_keras_npz(_npz(tmp_path, bad, arrays), wbits=4, abits=4)
            assert name in str(err.value)
    bad = [layers[0], _layer("Conv2D", "g0", "in", filters=8, groups=2, batch_input_shape=[None, 8, 8, 9], **COMMON)]
    with pytest.raises(ValueError, match="g0"):
        nets.spec_from_keras_npz(_npz(tmp_path, bad, arrays))
    with pytest.raises(ValueError, match="wbits"):
        nets.spec_from_keras_npz(_npz(tmp_path, [layers[0], _layer("QuantizedConv2D", "g1", "in", filters=8, groups=4, **COMMON)],
                                      arrays))
    # the new class serialises `nb`: such a config needs no wbits; without `nb` it does
    own = [layers[0], _layer("QuantizedGroupedConv2D", "g6", "in", filters=8, groups=2, nb=8, **COMMON)]
    assert nets.spec_from_keras_npz(_npz(tmp_path, own, arrays))[0]["nb"] == 8
    assert nets.spec_from_keras_npz(_npz(tmp_path, own, arrays), wbits=4, abits=4)[0]["nb"] == 8
    bare = [layers[0], _layer("QuantizedGroupedConv2D", "g6", "in", filters=8, groups=2, **COMMON)]
    assert nets.spec_from_keras_npz(_npz(tmp_path, bare, arrays), wbits=4, abits=4)[0]["nb"] == 4
    with pytest.raises(ValueError, match="g6.*wbits"):
        nets.spec_from_keras_npz(_npz(tmp_path, bare, arrays))


def test_importer_leaves_ungrouped_configs_as_they_were(tmp_path):
    rs = np.random.RandomState(4)
    arrays = {"c/kernel": rs.rand(3, 3, 8, 8).astype(np.float32), "c/bias": rs.rand(8).astype(np.float32)}
    for cls, kind in (("Conv2D", "float"), ("BinaryConv2D", "binary"), ("QuantizedConv2D", "quantized"), ("TernaryConv2D", "ternary")):
        specs = []
        for extra in ({}, {"groups": 1}):
            layers = [_layer("InputLayer", "in", None), _layer(cls, "c", "in", filters=8, **dict(COMMON, **extra))]
            specs.append(nets.spec_from_keras_npz(_npz(tmp_path, layers, arrays), wbits=4, abits=4))
        for spec in specs:
            assert len(spec) == 1 and spec[0]["op"] == "conv" and spec[0]["kind"] == kind and "groups" not in spec[0]
        assert sorted(specs[0][0]) == sorted(specs[1][0])
        for key in specs[0][0]:
            np.testing.assert_array_equal(specs[0][0][key], specs[1][0][key])
        want = {"op", "kind", "kernel", "bias", "strides", "padding", "klm", "src", "dst"}
        want |= {"nb"} if kind == "quantized" else {"H"} if kind == "ternary" else set()
        assert set(specs[0][0]) == want


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_header_symbols_and_prototypes():
    inc = os.path.join(ROOT, "include")
    text = open(os.path.join(inc, "qnn_abi_gconv.h")).read()
    for name in ENTRIES:
        assert name + "(" in text
    assert len(ENTRIES) == 5 and "qnn_gconv" not in open(os.path.join(inc, "qnn_abi.h")).read()
    assert "QNN_GC_MAX_WINDOW 7" in text and _abi.GC_MAX_WINDOW == 7 == G.MAX_WINDOW
    assert os.path.exists(_abi.lib_path()), "the library is not built"
    lib = _abi.load()
    assert lib.qnn_version() == 4
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert lib.qnn_gconv_prepack.argtypes == [ci, ci, ctypes.c_float, vp, ci, ci, ci, ci, ci, vp, ci, ci, ci, ci, ci, vp,
                                              ctypes.POINTER(vp)]
    assert lib.qnn_gconv_forward.argtypes == [vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(_abi.Epilogue), vp, vp]
    assert lib.qnn_gconv_out_hw.argtypes == [vp, ci, ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    assert lib.qnn_gconv_free.argtypes == [vp] and lib.qnn_gconv_dequant.argtypes == [vp, vp, vp]
    # the calls that need no device: null handles are refused, a null free is fine
    assert lib.qnn_gconv_free(None) == 0
    ho, wo = ci(0), ci(0)
    assert lib.qnn_gconv_out_hw(None, 4, 4, ctypes.byref(ho), ctypes.byref(wo)) == -1
