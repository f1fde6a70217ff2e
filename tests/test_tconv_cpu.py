"""The transposed convolution without a GPU: the numpy reference of tconv_cases.py against torch's conv_transpose2d in
float64 on every case geometry, the output-size rule against a table written out by hand (C header in a stand-alone
sanitized program, the reference and the binding), the route rule and the int32 refusal bound restated, the importer on a
hand-built .npz, and the planner's NotFusable / fallback."""
import itertools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import qnn_amd                                   # noqa: F401  (the package alias of conftest.py)
from qnn_amd import _abi, engine, nets

import depthwise_cases as D
import tconv_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quantizedneuralnetworks-keras-tensorflow_amd", "csrc")
ENTRIES = _abi.EXPORTS_TCONV                     # read at import: without the feature nothing below means anything

MAIN = r"""
#include <stdio.h>
#include "qnn_conv_geom.h"
int main() {
    int in, k, s, same;
    while (scanf("%d %d %d %d", &in, &k, &s, &same) == 4) {
        int out = -12345, before = -12345;
        qnn_tconv_out_pad(in, k, s, same, &out, &before);
        printf("%d %d\n", out, before);
    }
    return 0;
}
"""

GRID = list(itertools.product(range(1, 12), range(1, 9), range(1, 5), (0, 1)))      # (in, k, s, same)


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("tconv_geom")
    src, exe = d / "tconv_geom_main.cpp", d / "tconv_geom_main"
    src.write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    text = "".join("%d %d %d %d\n" % c for c in GRID)
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
    out = [tuple(int(v) for v in ln.split()) for ln in out if ln]
    assert len(out) == len(GRID)
    return dict(zip(GRID, out))


def test_output_size_table_written_by_hand(rule):
    n = T.SIZE_TABLE_IN
    assert set(T.SIZE_TABLE) == set(itertools.product((1, 2, 3, 4, 5, 8), (1, 2, 3, 4)))
    for (k, s), (valid_out, same_before) in T.SIZE_TABLE.items():
        assert T.out_pad(n, k, s, False) == (valid_out, 0), (k, s)
        assert T.out_pad(n, k, s, True) == (n * s, same_before), (k, s)
        assert rule[(n, k, s, 0)] == (valid_out, 0), (k, s)
        assert rule[(n, k, s, 1)] == (n * s, same_before), (k, s)
        assert _abi.tconv_out_hw(n, k, s, False) == valid_out and _abi.tconv_out_hw(n, k, s, True) == n * s
    # k < s under 'valid': the output is longer than the scatter, the rest is sums over no tap
    assert T.out_pad(5, 1, 3, False)[0] == 15 > (5 - 1) * 3 + 1


def test_header_and_reference_agree_on_the_grid(rule):
    """The C function against the statement of the rule: 'same' inverts the forward SAME convolution (out cells map back
    to `in`, its leading padding is ours), 'valid' is in * s + max(k - s, 0)."""
    for case in GRID:
        n, k, s, same = case
        out, before = rule[case]
        assert (out, before) == T.out_pad(n, k, s, bool(same)), case
        if same:
            assert out == n * s and -(-out // s) == n
            assert before == max((n - 1) * s + k - out, 0) // 2            # forward SAME padding on `out` cells
        else:
            assert out == n * s + max(k - s, 0) and before == 0
            assert out >= (n - 1) * s + k                                  # the whole scatter is kept


ALL_CASES = T.geometry_cases() + T.channel_cases() + T.mfma_cases() + T.boundary_cases() + T.multitask_cases()
GEOMETRIES = sorted({(c["window"], c["stride"], c["same"], c["map"]) for c in ALL_CASES})


def test_reference_sum_equals_torch_conv_transpose2d_on_every_case_geometry():
    rs = np.random.RandomState(11)
    for (kh, kw), s, same, (N, H, W) in GEOMETRIES:
        cin, cout = 3, 2
        x = rs.randint(-64, 65, (N, H, W, cin)) / 64.0
        w = rs.randint(-64, 65, (kh, kw, cout, cin)) / 64.0
        got = T.tconv_sum(x, w, s, same, np.float64)
        full = torch.nn.functional.conv_transpose2d(torch.from_numpy(x).permute(0, 3, 1, 2),
                                                    torch.from_numpy(w).permute(3, 2, 0, 1).contiguous(), stride=s)
        full = full.permute(0, 2, 3, 1).numpy()
        assert full.shape[1:3] == ((H - 1) * s + kh, (W - 1) * s + kw)
        # cut or zero-extend by the rule, written here a second time: per output cell, the cell of `full` or nothing
        Ho = H * s + (0 if same else max(kh - s, 0))
        Wo = W * s + (0 if same else max(kw - s, 0))
        pt = max(kh - s, 0) // 2 if same else 0
        pl = max(kw - s, 0) // 2 if same else 0
        want = np.zeros((N, Ho, Wo, cout))
        for oy in range(Ho):
            for ox in range(Wo):
                if oy + pt < full.shape[1] and ox + pl < full.shape[2]:
                    want[:, oy, ox] = full[:, oy + pt, ox + pl]
        assert got.shape == want.shape, ((kh, kw), s, same)
        np.testing.assert_array_equal(got, want, err_msg=str(((kh, kw), s, same, (N, H, W))))


def test_the_case_tables_cover_what_they_claim():
    geo = T.geometry_cases()
    for store in T.STORES:
        mine = [c for c in geo if c["store"] == store]
        assert {(c["window"], c["stride"], c["same"]) for c in mine} == set(itertools.product(T.WINDOWS, T.STRIDES, (True, False)))
        assert {c["map"] for c in mine} == set(T.MAPS) and {c["Cin"] for c in mine} == set(T.CINS)
        assert {c["Cout"] for c in mine} == set(T.COUTS)
    assert any(c["window"][0] < c["stride"] for c in geo) and any(c["window"][0] % c["stride"] for c in geo)
    m = T.mfma_cases()
    assert all(T.takes_mfma(c) for c in m) and not any(T.takes_mfma(c) for c in T.boundary_cases())
    assert not any(T.takes_mfma(c) for c in geo + T.channel_cases() + T.weight_cases() + T.epilogue_cases())
    for store, k, same in itertools.product((T.I4, T.I8), (2, 3, 4), (True, False)):
        mine = [c for c in m if (c["store"], c["window"], c["same"]) == (store, (k, k), same)]
        assert {c["map"] for c in mine} == set(T.MFMA_MAPS)
        assert {(c["Cin"], c["Cout"]) for c in mine} == {(64, 16), (128, 48)}


# ---- the multitask table: what it reaches, and that its expected values can tell pixel mappings apart ------------------------
FILL = 0x5A5A5A5A                                # what test_gpu_tconv.py lays under every output


def test_multitask_table_reaches_the_decodes_it_names():
    cases = T.multitask_cases()
    assert len({T.case_id(c) for c in cases}) == len(cases) == 19 and all(c["map"][0] >= 2 for c in cases)
    fast = [c for c in cases if T.takes_mfma(c)]
    assert len(fast) == 17
    for store in (T.I4, T.I8):
        for k, same, m in T.MULTITASK_MAPS:
            mine = [c for c in fast if (c["store"], c["window"], c["same"], c["map"]) == (store, (k, k), same, m)]
            assert {(c["Cin"], c["Cout"]) for c in mine} == {(64, 16), (128, 48)}          # FB = 1 half filled, FB = 2
    # the phases and the task count, restated from the map alone
    by_geom = {(3, False, (2, 2, 21)): ([66, 63, 44, 42], 2), (3, True, (2, 4, 40)): ([160] * 4, 3),
               (2, False, (2, 2, 21)): ([42] * 4, 1), (4, False, (2, 2, 21)): ([66] * 4, 2), (3, True, (70, 1, 1)): ([1] * 4, 1)}
    for c in fast:
        N, H, W = c["map"]
        k = c["window"][0]
        Ho, Wo = (v * 2 + (0 if c["same"] else max(k - 2, 0)) for v in (H, W))
        phases = [(Ho + 1) // 2 * ((Wo + 1) // 2), (Ho + 1) // 2 * (Wo // 2), Ho // 2 * ((Wo + 1) // 2), Ho // 2 * (Wo // 2)]
        GT, waves = T.wave_tasks(c)
        assert (T.phase_pixels(c), GT) == (phases, -(-(-(-phases[0] // 16)) // 4)) == by_geom[(k, c["same"], c["map"])]
        assert sum(phases) == Ho * Wo and waves == N * 4 * GT * -(-c["Cout"] // 32)
    # a phase that ends at or before the first group of a later task, so that task returns early with g0 > 0
    assert any(T.wave_tasks(c)[0] >= 2 and min(T.phase_pixels(c)) <= 16 * T.K_PG for c in fast)
    assert max(T.wave_tasks(c)[0] for c in fast) >= 3
    assert any(c["map"] == D.TINY_MAP and T.wave_tasks(c)[1] == 280 for c in fast)
    # the plain form past one workgroup at V = 4, and the same case at V = 1
    plain = [c for c in cases if not T.takes_mfma(c)]
    assert [c["misalign"] for c in plain] == [False, True] and all((c["store"], c["stride"]) == (T.I8, 2) for c in plain)
    items = [D.plain_items(c["out_store"], c["Cout"], 2 * 10 * 18, c["misalign"]) for c in plain]
    assert items == [(4, 360), (1, 1440)] and items[0][1] > D.BLOCK and items[0][1] % D.BLOCK


@pytest.mark.parametrize("c", T.multitask_cases(), ids=T.case_id)
def test_multitask_expected_values_tell_pixel_mappings_apart(c):
    """At most half of the codes at the clip ends, no two images and no two 16-pixel groups of an image alike -- the groups
    of the matrix-pipe form run over one phase --, and no expected word equal to the pattern the GPU test lays under the
    output."""
    want = T.reference(c, *T.make_inputs(c, c["seed"]))
    assert D.degenerate(c, want) == []
    if T.takes_mfma(c):
        assert D.degenerate(c, want, T.phase_groups(c, want)) == []
    assert not (T.encode(want, c["out_store"]) == FILL).any()


def test_route_rule_restated():
    base = T._case(T.I4, 64, 16, window=(3, 3), stride=2, map=(3, 2, 15))
    assert T.takes_mfma(base)
    for change in (dict(Cin=32), dict(Cin=96), dict(Cout=8), dict(Cout=24), dict(stride=1), dict(stride=3),
                   dict(window=(5, 5)), dict(window=(1, 1)), dict(window=(2, 3)), dict(out_store=T.I8), dict(out_store=T.F32),
                   dict(misalign=True), dict(Cin=16384 + 64)):
        assert not T.takes_mfma(dict(base, **change)), change
    for c in T.mfma_cases() + T.boundary_cases() + [base]:
        kh, kw = c["window"]
        assert T.takes_mfma(c) == _abi.tconv_takes_mfma(kh, kw, c["stride"], c["store"], c["Cout"], c["Cin"], c["out_store"])
    assert not T.takes_mfma(T._case(T.BIN, 64, 16)) and not T.takes_mfma(T._case(T.T2, 64, 16))


def test_int32_refusal_bound_at_its_edge():
    # 8-bit codes x 8-bit weights, 2x2 at stride 2: one tap per output, 2^14 per pair -> Cin = 2^17 is the first refused
    assert not T.int32_refused(2, 2, 2, (1 << 17) - 1, 8, 7) and T.int32_refused(2, 2, 2, 1 << 17, 8, 7)
    # 4x4 at stride 2: four taps -> a quarter of it; at stride 1: sixteen
    assert not T.int32_refused(4, 4, 2, (1 << 15) - 1, 8, 7) and T.int32_refused(4, 4, 2, 1 << 15, 8, 7)
    assert not T.int32_refused(4, 4, 1, (1 << 13) - 1, 8, 7) and T.int32_refused(4, 4, 1, 1 << 13, 8, 7)
    # ceil, not floor: 3x3 at stride 2 counts 2 x 2 taps, 5x5 at stride 4 too
    assert T.int32_refused(3, 3, 2, 1 << 15, 8, 7) and T.int32_refused(5, 5, 4, 1 << 15, 8, 7)
    assert not T.int32_refused(1, 1, 4, 1 << 16, 8, 7)
    # no shape of the matrix-pipe form (Cin <= 16384) is refused, and its code * 16 int4 operands stay below 2^31 too
    assert not T.int32_refused(4, 4, 2, 16384, 8, 7)
    assert 2 * 2 * 16384 * 8 * 8 * 16 < (1 << 31)


# ---- the importer ----------------------------------------------------------------------------------------------------------
def _npz(tmp_path, layers, arrays):
    cfg = {"class_name": "Model", "config": {"layers": layers}}
    path = str(tmp_path / "net.npz")
    np.savez(path, model_config_json=np.frombuffer(json.dumps(cfg).encode(), np.uint8), **arrays)
    return path


def _layer(cls, name, src, **config):
    return {"class_name": cls, "name": name, "config": dict(config, name=name), "inbound_nodes": [[[src, 0, 0, {}]]] if src else []}


def test_importer_maps_the_four_classes_and_refuses_the_rest(tmp_path):
    rs = np.random.RandomState(2)
    common = dict(padding="same", data_format="channels_last", activation="linear", use_bias=True, output_padding=None,
                  dilation_rate=[1, 1])
    names = [("Conv2DTranspose", "up0", "float"), ("BinaryConv2DTranspose", "up1", "binary"),
             ("QuantizedConv2DTranspose", "up2", "quantized"), ("TernaryConv2DTranspose", "up3", "ternary")]
    arrays, layers, src, cin = {}, [_layer("InputLayer", "in", None)], "in", 3
    for cls, name, kind in names:
        arrays[name + "/kernel"] = rs.rand(2, 2, 4, cin).astype(np.float32)
        arrays[name + "/bias"] = rs.rand(4).astype(np.float32)
        extra = {} if kind == "float" else {"H": 1.0, "kernel_lr_multiplier": 2.5}
        if kind == "ternary":
            extra["H"] = 0.5
        layers.append(_layer(cls, name, src, filters=4, kernel_size=[2, 2], strides=[2, 2], **dict(common, **extra)))
        src, cin = name, 4
    spec = nets.spec_from_keras_npz(_npz(tmp_path, layers, arrays), wbits=4, abits=4)
    assert [op["op"] for op in spec] == ["tconv"] * 4
    assert [op["kind"] for op in spec] == ["float", "binary", "quantized", "ternary"]
    assert spec[0]["src"] == "input" and spec[1]["src"] == "up0" and [op["dst"] for op in spec] == ["up0", "up1", "up2", "up3"]
    assert spec[2]["nb"] == 4 and spec[3]["H"] == 0.5 and spec[0]["H"] == 1.0
    assert all(op["klm"] == np.float32(2.5) for op in spec[1:]) and spec[0]["klm"] == np.float32(1.0)
    for op, (_, name, _) in zip(spec, names):
        assert op["strides"] == (2, 2) and op["padding"] == "same"
        np.testing.assert_array_equal(op["kernel"], arrays[name + "/kernel"])
        np.testing.assert_array_equal(op["bias"], arrays[name + "/bias"])
    no_bias = [layers[0], _layer("Conv2DTranspose", "up0", "in", filters=4, kernel_size=[2, 2], strides=[2, 2],
                                 **dict(common, use_bias=False))]
    assert nets.spec_from_keras_npz(_npz(tmp_path, no_bias, arrays))[0]["bias"] is None
    for cls, name, _ in names:
        for change, match in ((dict(activation="relu"), "activation"), (dict(output_padding=[1, 1]), "output_padding"),
                              (dict(dilation_rate=[2, 2]), "dilation_rate"), (dict(data_format="channels_first"), "channels_first")):
            bad = [layers[0], _layer(cls, name, "in", filters=4, kernel_size=[2, 2], strides=[2, 2], **dict(common, **change))]
            with pytest.raises(ValueError, match=match) as err:
                nets.spec_from_keras_npz(_npz(tmp_path, bad, arrays), wbits=4, abits=4)
            assert name in str(err.value)


# ---- the planner -----------------------------------------------------------------------------------------------------------
def test_fused_engines_decline_and_the_layer_classes_refuse_what_the_entry_lacks():
    spec = [{"op": "tconv", "kind": "quantized", "nb": 4, "kernel": np.zeros((2, 2, 16, 64), np.float32), "bias": None,
             "strides": (2, 2), "padding": "same", "H": 1.0}]
    for cls in (engine.FusedModel, engine.ResidualFusedModel):
        with pytest.raises(_abi.NotFusable, match="tconv.*GraphModel"):
            cls(spec, "cpu")
    for kw in (dict(output_padding=1), dict(output_padding=(1, 1)), dict(dilation_rate=2), dict(data_format="channels_first"),
               dict(strides=5), dict(strides=(1, 2))):
        for cls in (qnn_amd.Conv2DTranspose, qnn_amd.BinaryConv2DTranspose, qnn_amd.QuantizedConv2DTranspose,
                    qnn_amd.TernaryConv2DTranspose):
            with pytest.raises(_abi.QnnError):
                cls(8, (2, 2), **kw)
    with pytest.raises(_abi.QnnError):
        qnn_amd.Conv2DTranspose(8, (9, 9))
    layer = qnn_amd.QuantizedConv2DTranspose(8, 3, strides=2, padding="same", nb=4)
    assert layer.compute_output_shape((2, 5, 7, 3)) == (2, 10, 14, 8)
    assert qnn_amd.Conv2DTranspose(8, (2, 5), strides=3).compute_output_shape((2, 5, 7, 3)) == (2, 15, 23, 8)
    cfg = layer.get_config()
    assert cfg["filters"] == 8 and cfg["kernel_size"] == (3, 3) and cfg["strides"] == (2, 2) and cfg["nb"] == 4
    assert cfg["output_padding"] is None and cfg["dilation_rate"] == (1, 1)


def test_abi_header_and_version_are_what_they_were():
    inc = os.path.join(ROOT, "include")
    text = open(os.path.join(inc, "qnn_abi_tconv.h")).read()
    for name in ENTRIES:
        assert name + "(" in text
    assert "qnn_tconv" not in open(os.path.join(inc, "qnn_abi.h")).read()
    assert "QNN_TC_MAX_WINDOW 8" in text and _abi.TC_MAX_WINDOW == 8 == T.MAX_WINDOW and _abi.TC_MAX_STRIDE == 4 == T.MAX_STRIDE
    if os.path.exists(_abi.lib_path()):
        assert _abi.load().qnn_version() == 4
