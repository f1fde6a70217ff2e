#!/usr/bin/env python3
"""Compare the gfx950 assembly of two source trees kernel by kernel (no GPU needed): the check of a refactor that is
meant to leave the compiled kernels as they are, where byte-identical assembly is too much to ask.

    git archive HEAD~ | tar -x -C /tmp/parent
    python tools/asm_compare.py /tmp/parent . --out /tmp/asm [--loops qnn_mfma_strip,qnn_mfma_strip_dil,...]

Every csrc/*.hip of both trees is compiled with _build.py's flags plus `-cuid=asmcompare --cuda-device-only -S` (the
fixed cuid keeps the suffixes of the internal-linkage kernels equal; .ident / .file lines are dropped) into
<out>/parent/*.s and <out>/branch/*.s; a file that is already there is reused.  Printed as markdown tables:
  * per file: diff lines, kernels in either tree, whether the sorted kernel-name lists are equal;
  * for the files named by --loops, per kernel: the resource figures (next_free_vgpr / next_free_sgpr / accum_offset,
    scratch, LDS, Occupancy) and three regions compared by class counts (tools/isa_count.py) and opcode histogram:
      loop  every innermost loop that contains MFMAs (header .. back edge in layout order),
      tail  every other block that holds an MFMA, wherever the compiler laid it out (the unrolled remainder rows behind or
            between the loops, a row computed ahead of the loop), as one sum,
      rest  everything else (once-per-wave preamble, per-task setup): reported, not required to be equal;
  * per file the difference of the whole-file opcode histogram.
Exit status 1 when a name list, a resource figure or a loop / tail region differs.
"""
import argparse
import collections
import concurrent.futures
import difflib
import glob
import importlib.util
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_count  # noqa: E402

PKG = "quantizedneuralnetworks-keras-tensorflow_amd"
FIGURES = (r"\.amdhsa_next_free_vgpr\s+(\S+)", r"\.amdhsa_next_free_sgpr\s+(\S+)", r"\.amdhsa_accum_offset\s+(\S+)",
           r";\s*ScratchSize:\s*(\S+)", r";\s*LDSByteSize:\s*(\S+)", r";\s*Occupancy:\s*(\S+)")


def compile_tree(tree, out, jobs):
    # each tree is compiled with the flags of its OWN _build.py (a change of CFLAGS then shows up as a difference)
    spec = importlib.util.spec_from_file_location("_build_" + os.path.basename(out), os.path.join(tree, PKG, "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    os.makedirs(out, exist_ok=True)
    flags = [f for f in b.CFLAGS if not f.startswith("-I")] + ["-I" + os.path.join(tree, "include"),
                                                               "-I" + os.path.join(tree, PKG, "csrc")]

    def one(src):
        dst = os.path.join(out, os.path.basename(src)[:-4] + ".s")
        if not os.path.exists(dst):
            r = subprocess.run([b._hipcc()] + flags + ["-cuid=asmcompare", "--cuda-device-only", "-S", src, "-o", "-"],
                               check=True, capture_output=True, text=True)
            with open(dst, "w") as f:
                f.writelines(ln + "\n" for ln in r.stdout.splitlines() if not re.match(r"^\s*\.(ident|file)", ln))
        return dst

    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        return {os.path.basename(p)[:-2]: p for p in ex.map(one, sorted(glob.glob(os.path.join(tree, PKG, "csrc", "*.hip"))))}


def kernels_of(asm):
    """{name: (figures, body lines)} of every .amdhsa_kernel of the file."""
    lines = asm.splitlines()
    out = {}
    label = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"^(_Z\w+):", ln)] if m}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M):
        i = label[name]
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        stop = next((j for j in range(end + 1, len(lines)) if re.match(r"^_Z\w+:", lines[j])), len(lines))
        text = "\n".join(lines[i:stop])               # (the .amdhsa_ block precedes .Lfunc_end, the comments follow it)
        figs = tuple((re.search(p, text) or [None, "-"])[1] for p in FIGURES)
        out[name] = (figs, lines[i + 1:end])
    return out


def hist(insts):
    return collections.Counter(re.sub(r"_e(32|64)$", "", op) for op, _ in insts)


def regions(body):
    """(loops, tail, rest): class counts and opcode histogram of each innermost MFMA loop, of all other blocks that
    hold an MFMA, and of everything else."""
    blocks = isa_count.blocks_of(body)
    index = {lab: i for i, (lab, _, _) in enumerate(blocks)}
    loops = sorted({(index[t], i) for i, (_, _, br) in enumerate(blocks) for t in br if t in index and index[t] <= i})
    has_mfma = lambda h, e: any(isa_count.classify(op) == "MFMA" for i in range(h, e + 1) for op, _ in blocks[i][1])
    inner = [(h, e) for h, e in loops if has_mfma(h, e) and
             not any((h2, e2) != (h, e) and h <= h2 and e2 <= e and has_mfma(h2, e2) for h2, e2 in loops)]
    taken = set()
    loop_sets = []
    for h, e in inner:
        taken.update(range(h, e + 1))
        loop_sets.append([x for i in range(h, e + 1) for x in blocks[i][1]])
    is_mfma = lambda blk: any(isa_count.classify(op) == "MFMA" for op, _ in blk[1])
    tail = [i for i in range(len(blocks)) if i not in taken and is_mfma(blocks[i])]
    taken.update(tail)
    rest = [x for i in range(len(blocks)) if i not in taken for x in blocks[i][1]]
    fold = lambda insts: (tuple(isa_count.counts(insts)), hist(insts))
    return [fold(x) for x in loop_sets], fold([x for i in tail for x in blocks[i][1]]), fold(rest)


def hist_diff(a, b):
    d = {k: b[k] - a[k] for k in set(a) | set(b) if a[k] != b[k]}
    return ", ".join("%s %+d" % kv for kv in sorted(d.items())) or "none"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--out", required=True, help="directory for the .s files (kept out of git)")
    ap.add_argument("--loops", default="", help="comma-separated files (without .hip) compared kernel by kernel")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--verbose", action="store_true", help="one row per kernel, not only the kernels that differ")
    a = ap.parse_args()
    pa = compile_tree(os.path.abspath(a.parent), os.path.join(a.out, "parent"), a.jobs)
    br = compile_tree(os.path.abspath(a.branch), os.path.join(a.out, "branch"), a.jobs)
    bad = 0
    deep = [x for x in a.loops.split(",") if x]

    print("| file | diff lines | kernels parent / branch | names equal | whole-file opcode difference (branch - parent) |")
    print("|---|---|---|---|---|")
    parsed = {}
    for f in sorted(set(pa) | set(br)):
        if f not in pa or f not in br:
            print("| `%s` | only in %s | | | |" % (f, "parent" if f in pa else "branch"))
            continue
        ta, tb = open(pa[f]).read(), open(br[f]).read()
        nd = 0 if ta == tb else sum(1 for ln in difflib.unified_diff(ta.splitlines(), tb.splitlines(), lineterm="", n=0)
                                    if ln[:1] in "+-" and ln[:3] not in ("+++", "---"))
        ka, kb = kernels_of(ta), kernels_of(tb)
        same = sorted(ka) == sorted(kb)
        bad += not same or (nd != 0 and f not in deep)
        ha = hist(x for _, body in ka.values() for lab, insts, _ in isa_count.blocks_of(body) for x in insts)
        hb = hist(x for _, body in kb.values() for lab, insts, _ in isa_count.blocks_of(body) for x in insts)
        print("| `%s` | %d | %d / %d | %s | %s |" % (f, nd, len(ka), len(kb), "yes" if same else "NO", hist_diff(ha, hb)))
        parsed[f] = (ka, kb)

    for f in deep:
        ka, kb = parsed[f]
        rows, nres, nloop, ntail, nrest, worst = [], 0, 0, 0, 0, 0
        for name in sorted(set(ka) & set(kb)):
            (fa, ba), (fb, bb) = ka[name], kb[name]
            la, ta, ra = regions(ba)
            lb, tb, rb = regions(bb)
            res_ok, loop_ok, tail_ok = fa == fb, la == lb, ta == tb
            nres += not res_ok
            nloop += not loop_ok
            ntail += not tail_ok
            rest = hist_diff(ra[1], rb[1])
            nrest += rest != "none"
            worst = max(worst, sum(abs(rb[1][k] - ra[1][k]) for k in set(ra[1]) | set(rb[1])))
            if a.verbose or not (res_ok and loop_ok and tail_ok):
                rows.append("| `%s` | %s | %s | %s | %s | %s |" % (
                    name, " ".join(fa) + ("" if res_ok else " -> " + " ".join(fb)),
                    "; ".join("%d/%d/%d/%d/%d" % c for c, _ in la) or "-",
                    "equal" if loop_ok else "DIFFERS: " + "; ".join(hist_diff(x[1], y[1]) for x, y in zip(la, lb)),
                    "equal" if tail_ok else "DIFFERS: " + hist_diff(ta[1], tb[1]), rest))
        bad += nres + nloop + ntail
        print("\n### `%s`: %d kernels; resource figures differ in %d, MFMA loops in %d, remainder rows in %d; "
              "%d differ outside the loops (largest sum of |opcode differences| in one kernel: %d)\n"
              % (f, len(ka), nres, nloop, ntail, nrest, worst))
        if rows:
            print("| kernel | vgpr sgpr accum scratch lds occupancy | loops VALU/MFMA/LDS/VMEM/SALU | loops | remainder | outside |")
            print("|---|---|---|---|---|---|")
            print("\n".join(rows))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
