#!/usr/bin/env python3
"""Instruction counts of one kernel from the gfx950 assembly of one csrc/*.hip file (no GPU needed).

    python tools/isa_count.py qnn_mfma_areg.hip k_conv_mfma_haloILi8ELi8ELb0ELb1ELb1E
    python tools/isa_count.py qnn_mfma_areg.hip haloILi4ELi8ELb1ELb1ELb0E --hist .LBB31_25,.LBB31_26

The file is compiled with _build.py's flags plus --cuda-device-only -S (or read from --asm FILE).  For the kernel whose
mangled name contains the given substring it prints
  * VGPRs, scratch bytes and occupancy (the compiler's own figures),
  * one row per basic block: VALU / MFMA / LDS / VMEM / SALU instructions and where the block branches to,
  * one row per loop (a backward branch): the sums over the blocks from its header to its back edge in layout order --
    blocks of both sides of a branch inside the loop are all counted, a path's count is the sum of its block rows,
  * for the block with the most MFMAs: v_mov_b32 between its first and last MFMA, `v_max_f32 v, x, x` canonicalisations,
    v_min* and v_cndmask counts, and the opcode histogram.  --hist takes other blocks (comma-separated: a path).
"""
import argparse
import collections
import importlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("VALU", "MFMA", "LDS", "VMEM", "SALU")


def classify(op):
    if op.startswith(("v_mfma", "v_smfmac")):
        return "MFMA"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_", "tbuffer_")):
        return "VMEM"
    if op.startswith("s_"):
        return "SALU"
    return None


def assembly(src):
    sys.path.insert(0, ROOT)
    b = importlib.import_module("quantizedneuralnetworks-keras-tensorflow_amd._build")
    path = src if os.path.exists(src) else os.path.join(b.CSRC, src)
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([b._hipcc()] + b.CFLAGS + ["--cuda-device-only", "-S", path, "-o", out], check=True)
        return open(out).read()


def kernel_text(asm, sub):
    """(name, body lines, trailer lines with the compiler's resource comments) of the first kernel matching sub."""
    lines = asm.splitlines()
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m and sub in m.group(1):
            name = m.group(1)
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            trailer = []
            for j in range(end, min(end + 80, len(lines))):
                if j > end and re.match(r"^_Z\w+:", lines[j]):
                    break
                trailer.append(lines[j])
            return name, lines[i + 1:end], trailer
    raise SystemExit("no kernel whose mangled name contains %r" % sub)


def blocks_of(body):
    """[(label, [(opcode, operands)], [branch targets])] in layout order."""
    blocks = [("entry", [], [])]
    for ln in body:
        m = re.match(r"^(\.LBB\d+_\d+):", ln) or re.match(r"^; (%bb\.\d+):", ln)     # (fall-through blocks carry no label)
        if m:
            blocks.append((m.group(1), [], []))
            continue
        s = ln.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        op, _, rest = s.partition(" ")
        if classify(op) is None:
            continue
        blocks[-1][1].append((op, rest.strip()))
        if op.startswith(("s_cbranch", "s_branch")):
            blocks[-1][2].append(rest.strip())
    return blocks


def counts(insts):
    c = collections.Counter(classify(op) for op, _ in insts)
    return [c[k] for k in CLASSES]


def self_max(insts):
    n = 0
    for op, rest in insts:
        a = [x.strip() for x in rest.split(",")]
        if op in ("v_max_f32_e32", "v_max_f32_e64", "v_max_f32") and len(a) == 3 and a[1] == a[2]:
            n += 1
    return n


def detail(title, insts):
    print("\n%s: %d instructions" % (title, len(insts)))
    mf = [i for i, (op, _) in enumerate(insts) if classify(op) == "MFMA"]
    if mf:
        inner = insts[mf[0]:mf[-1] + 1]
        print("  v_mov_b32 between the first and the last MFMA: %d" % sum(op.startswith("v_mov_b32") for op, _ in inner))
    print("  v_max_f32 v, x, x: %d   v_min*: %d   v_cndmask*: %d   v_cvt_i32_f32: %d" % (
        self_max(insts), sum(op.startswith("v_min") for op, _ in insts),
        sum(op.startswith("v_cndmask") for op, _ in insts), sum(op.startswith("v_cvt_i32_f32") for op, _ in insts)))
    hist = collections.Counter(re.sub(r"_e(32|64)$", "", op) for op, _ in insts)
    for op, n in sorted(hist.items(), key=lambda kv: (-kv[1], kv[0])):
        print("  %4d  %s" % (n, op))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", help="a file of csrc/ (name or path)")
    ap.add_argument("kernel", help="substring of the mangled kernel name")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--hist", help="blocks for the opcode histogram (comma-separated labels) instead of the MFMA block")
    ap.add_argument("--save-asm", help="write the kernel's assembly here")
    a = ap.parse_args()

    asm = open(a.asm).read() if a.asm else assembly(a.source)
    name, body, trailer = kernel_text(asm, a.kernel)
    if a.save_asm:
        with open(a.save_asm, "w") as f:
            f.write("\n".join([name + ":"] + body + trailer) + "\n")
    print(name)
    for key in ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize"):
        for ln in trailer:
            m = re.match(r"^;\s*%s:\s*(\S+)" % key, ln)
            if m:
                print("  %-12s %s" % (key, m.group(1)))
                break

    blocks = blocks_of(body)
    index = {lab: i for i, (lab, _, _) in enumerate(blocks)}
    print("\n%-12s %5s %5s %5s %5s %5s  %s" % (("block",) + CLASSES + ("branches to",)))
    for lab, insts, br in blocks:
        print("%-12s %5d %5d %5d %5d %5d  %s" % ((lab,) + tuple(counts(insts)) + (" ".join(br),)))

    loops = sorted({(index[t], i) for i, (_, _, br) in enumerate(blocks) for t in br if t in index and index[t] <= i})
    if loops:
        print("\n%-25s %5s %5s %5s %5s %5s" % (("loop (header .. back edge)",) + CLASSES))
    for h, e in loops:
        tot = [sum(x) for x in zip(*(counts(blocks[i][1]) for i in range(h, e + 1)))]
        print("%-25s %5d %5d %5d %5d %5d" % (("%s .. %s" % (blocks[h][0], blocks[e][0]),) + tuple(tot)))

    if a.hist:
        labs = a.hist.split(",")
        detail(" + ".join(labs), [x for lab in labs for x in blocks[index[lab]][1]])
    else:
        lab, insts, _ = max(blocks, key=lambda b: counts(b[1])[1])
        detail(lab, insts)


if __name__ == "__main__":
    main()
