"""Instruction budget of k_conv_mfma_halo's EDGE staging in the two headline instantiations (CIFAR B0 <8, 8, false, FOLD, FP6,
EDGE> and C0 + classifier <4, 8, HEAD, FOLD, FP6, EDGE>), from the gfx950 assembly (tools/isa_count.py; no GPU).

The figure is the tile loop as the tool prints it: the VALU instructions of all blocks from the loop's header to its last
back edge (both epilogue paths are in it; the all-positive path of the headline is 75 / 184 of them).  Measured in the
assembly: 271 (B0; the general staging: 291) and 476 (C0; 516) -- profiles/halo_edge/README.md.  The ceilings are those
figures plus 2.  Both forms must keep two waves per SIMD without scratch.
"""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")

# mangled-name piece: (measured VALU of the tile loop, the same loop with the general staging)
EDGE = {"k_conv_mfma_haloILi8ELi8ELb0ELb1ELb1ELb1E": (271, 291), "k_conv_mfma_haloILi4ELi8ELb1ELb1ELb1ELb1E": (476, 516)}
GENERAL = {"k_conv_mfma_haloILi8ELi8ELb0ELb1ELb1ELb1E": "k_conv_mfma_haloILi8ELi8ELb0ELb1ELb1ELb0E",
           "k_conv_mfma_haloILi4ELi8ELb1ELb1ELb1ELb1E": "k_conv_mfma_haloILi4ELi8ELb1ELb1ELb1ELb0E"}


@pytest.fixture(scope="module")
def isa():
    spec = importlib.util.spec_from_file_location("isa_count", os.path.join(ROOT, "tools", "isa_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.assembly("qnn_mfma_areg.hip")


def _tile_loop(mod, asm, kernel):
    """(resources, class counts of the widest loop around the block with the most MFMAs, counts of that block)"""
    name, body, trailer = mod.kernel_text(asm, kernel)
    res = {}
    for ln in trailer:
        for key in ("NumVgprs", "ScratchSize", "Occupancy"):
            if ln.startswith("; %s:" % key):
                res[key] = int(ln.split(":")[1])
    blocks = mod.blocks_of(body)
    index = {lab: i for i, (lab, _, _) in enumerate(blocks)}
    m = max(range(len(blocks)), key=lambda i: mod.counts(blocks[i][1])[1])
    loops = [(index[t], i) for i, (_, _, br) in enumerate(blocks) for t in br if t in index and index[t] <= m <= i]
    assert loops, "the MFMA block of %s is in no loop" % name
    h, e = min(h for h, _ in loops), max(e for _, e in loops)
    tot = [sum(x) for x in zip(*(mod.counts(blocks[i][1]) for i in range(h, e + 1)))]
    return name, res, dict(zip(mod.CLASSES, tot)), dict(zip(mod.CLASSES, mod.counts(blocks[m][1])))


@pytest.mark.parametrize("kernel", sorted(EDGE), ids=["c0_classifier", "b0"])
def test_edge_tile_loop_budget(isa, kernel):
    mod, asm = isa
    measured, general = EDGE[kernel]
    name, res, loop, mfma_block = _tile_loop(mod, asm, kernel)
    _, res_g, loop_g, mfma_block_g = _tile_loop(mod, asm, GENERAL[kernel])
    print("\n[isa] %s: %s; tile loop: %s; with the general staging: %s" % (name, res, loop, loop_g))
    assert mfma_block["MFMA"] == 36 and loop["MFMA"] == 36                    # 9 taps x 4 tiles, once per tile
    assert mfma_block == mfma_block_g                                         # the MFMA loop is what it was
    assert loop["VALU"] <= measured + 2, loop
    assert loop_g["VALU"] <= general + 2, loop_g
    assert res["ScratchSize"] == 0 and res_g["ScratchSize"] == 0
    assert res["Occupancy"] == 2 and res["NumVgprs"] <= 256, res
