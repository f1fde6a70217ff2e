"""Instruction budget of the byte first layer's main loop, from the gfx950 assembly (tools/isa_count.py; no GPU).

The headline instantiation k_conv_first_u8<I4, 2, false, F32IN, FOLD> is bound by vector issue, so
its main-loop block -- two steps of 32 conv positions x 64 filters -- is held to a count: at most 118 VALU instructions
(137 before the filters were dealt to the MFMA columns and the image staging moved to running accumulators), no
ds_swizzle_b32 (the 8 x 8 nibble transpose is gone), no scratch, and registers for at least four waves per SIMD, which is
what the launcher's persistent grid of four 256-thread workgroups per CU keeps resident.
"""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")


@pytest.fixture(scope="module")
def isa():
    spec = importlib.util.spec_from_file_location("isa_count", os.path.join(ROOT, "tools", "isa_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.assembly("qnn_first_u8.hip")


def _loop(mod, asm, kernel):
    name, body, trailer = mod.kernel_text(asm, kernel)
    res = {}
    for ln in trailer:
        for key in ("NumVgprs", "ScratchSize", "Occupancy"):
            if ln.startswith("; %s:" % key):
                res[key] = int(ln.split(":")[1])
    blocks = mod.blocks_of(body)
    lab, insts, br = max(blocks, key=lambda b: mod.counts(b[1])[1])          # the block with the most MFMAs
    assert lab in br, "the MFMA block %s is not a loop of its own" % lab
    return res, dict(zip(mod.CLASSES, mod.counts(insts))), [op for op, _ in insts]


def test_headline_main_loop_budget(isa):
    mod, asm = isa
    res, cls, ops = _loop(mod, asm, "k_conv_first_u8ILi4ELi2ELb0ELb1ELb1E")
    print("\n[isa] f32-image fold form: %s; main loop per two steps: %s" % (res, cls))
    assert cls["MFMA"] == 16                                                  # two steps of 2 tiles x 4 filter blocks
    assert cls["VALU"] <= 118, cls
    assert res["ScratchSize"] == 0
    assert res["Occupancy"] >= 4 and res["NumVgprs"] <= 128, res               # four waves per SIMD stay possible
    assert not any(op.startswith("ds_swizzle") for op in ops)
    assert not any(op.startswith("v_pk_") and op.endswith("_f32") for op in ops)          # packed float32: dearer than two plain ones


@pytest.mark.parametrize("kernel", ["k_conv_first_u8ILi4ELi2ELb0ELb0ELb1E", "k_conv_first_u8ILi4ELi2ELb0ELb1ELb0E",
                                    "k_conv_first_u8ILi4ELi2ELb0ELb0ELb0E", "k_conv_first_u8ILi4ELi2ELb1ELb1ELb0E",
                                    "k_conv_first_u8ILi4ELi2ELb1ELb0ELb0E"],
                         ids=["fold_u8", "chain_f32", "chain_u8", "bin_f32", "bin_u8"])
def test_no_pooled_form_transposes_across_lanes(isa, kernel):
    mod, asm = isa
    res, cls, ops = _loop(mod, asm, kernel)
    print("\n[isa] %s: %s; main loop per two steps: %s" % (kernel, res, cls))
    assert cls["MFMA"] == 16 and res["ScratchSize"] == 0 and res["Occupancy"] >= 4
    assert not any(op.startswith("ds_swizzle") for op in ops)
    if kernel.endswith("Lb0ELb1E"):                                           # the byte-input fold form: item 1's share only
        assert cls["VALU"] <= 94, cls                                          # 102 before, minus the transpose (2 x 5)
