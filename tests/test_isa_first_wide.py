"""Instruction budget of the byte first layer's image-wide strip (k_conv_first_u8<..., SW = 32>), from the gfx950 assembly
(tools/isa_count.py; no GPU).

Its main-loop block is two steps of 64 conv positions x 64 filters: twice the positions of the 16-column form's block
(96 VALU for float32 images, 76 for bytes: profiles/first_tab/isa_first*.txt).  Measured in the assembly: 174 and 144
(profiles/first_wide/README.md); the ceilings are those figures plus 2, and the figures are below twice the narrow block's.
"""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")

# mangled-name piece of <I4, 2, false, F32IN, FOLD = true, TAB = 2, SW = 32>: (measured VALU of the block, narrow block)
WIDE = {"k_conv_first_u8ILi4ELi2ELb0ELb1ELb1ELi2ELi32E": (174, 96), "k_conv_first_u8ILi4ELi2ELb0ELb0ELb1ELi2ELi32E": (144, 76)}


@pytest.fixture(scope="module")
def isa():
    spec = importlib.util.spec_from_file_location("isa_count", os.path.join(ROOT, "tools", "isa_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.assembly("qnn_first_u8.hip")


@pytest.mark.parametrize("kernel", sorted(WIDE), ids=["u8", "f32_image"])
def test_wide_main_loop_budget(isa, kernel):
    mod, asm = isa
    measured, narrow = WIDE[kernel]
    assert measured < 2 * narrow
    name, body, trailer = mod.kernel_text(asm, kernel)
    res = {}
    for ln in trailer:
        for key in ("NumVgprs", "ScratchSize", "Occupancy"):
            if ln.startswith("; %s:" % key):
                res[key] = int(ln.split(":")[1])
    blocks = mod.blocks_of(body)
    lab, insts, br = max(blocks, key=lambda b: mod.counts(b[1])[1])          # the block with the most MFMAs
    assert lab in br, "the MFMA block %s is not a loop of its own" % lab
    cls = dict(zip(mod.CLASSES, mod.counts(insts)))
    print("\n[isa] %s: %s; main loop per two steps: %s" % (name, res, cls))
    assert cls["MFMA"] == 32                                                  # two steps of 4 tiles x 4 filter blocks
    assert cls["VALU"] <= measured + 2, cls
    assert res["ScratchSize"] == 0
    assert res["Occupancy"] >= 4 and res["NumVgprs"] <= 128, res               # four waves per SIMD stay possible
