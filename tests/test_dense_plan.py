"""The host plan of the register-fed dense GEMM (csrc/qnn_dense_plan.h) against its Python restatement in
dense_mfma_cases.py.  No GPU: the header is plain C++, compiled here with a small main of its own into a stand-alone program
under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dense_mfma_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quantizedneuralnetworks-keras-tensorflow_amd", "csrc")

# per input line "N units steps cus": "no", or "nt ks ublocks blocks"
MAIN = r"""
#include <stdio.h>
#include "qnn_dense_plan.h"
int main() {
    long N;
    int units, steps, cus;
    while (scanf("%ld %d %d %d", &N, &units, &steps, &cus) == 4) {
        DensePlan p;
        if (!dense_plan(&p, N, units, steps, cus)) printf("no\n");
        else printf("%d %d %d %u\n", p.nt, p.ks, p.ublocks, p.blocks);
    }
    return 0;
}
"""

NS = sorted(set(range(1, 71)) | {16 * k + d for k in range(5, 263) for d in (-1, 0, 1)} |
            {2 ** 14 + 1, 16401, 65535, 2 ** 17 - 15, 2 ** 20 - 1, 2 ** 20})
UNITS = tuple(range(16, 2065, 16))
STEPS = tuple(range(1, 21)) + (64, 72, 1024)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler: the plan header cannot be checked")
    d = tmp_path_factory.mktemp("dense_plan")
    src, exe = d / "plan_main.cpp", d / "plan_main"
    src.write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def run(cases):
        text = "".join("%d %d %d %d\n" % c for c in cases)
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
        out = [ln for ln in out if ln]
        assert len(out) == len(cases)
        return [None if ln == "no" else tuple(int(v) for v in ln.split()) for ln in out]
    return run


def _check(cases, got):
    """The header's answers against plans(), and the invariants the kernel relies on, on arrays."""
    assert all(g is not None for g in got)
    N, units, steps = (np.array(v, dtype=np.int64) for v in zip(*[c[:3] for c in cases]))
    nt, ks, ublocks, blocks = (np.array(v, dtype=np.int64) for v in zip(*got))
    ok, *want = M.plans(N, units, steps, cases[0][3])
    assert ok.all() and all(np.array_equal(g, w) for g, w in zip((nt, ks, ublocks, blocks), want)), cases[0]
    assert np.isin(nt, (1, 2, 4)).all() and np.isin(ks, (1, 2, 4)).all()
    assert (ublocks * nt * 16 >= units).all() and ((ublocks - 1) * nt * 16 < units).all()
    assert np.array_equal(blocks, ublocks * -(-(-(-N // 16)) // (4 // ks))) and (blocks > 0).all() and (blocks < 2 ** 31).all()
    share = -(-steps // ks)
    assert (share * ks >= steps).all() and ((share - 1) * ks < steps).all()       # the shares cover K; none but the last ones is short
    return set(zip(nt.tolist(), ks.tolist()))


@pytest.mark.parametrize("cus", [256, 1, 64])
def test_plan_matches_the_restatement_on_the_sweep(planner, cus):
    """The whole product of N, units and steps at 256 CUs; at 1 and 64 CUs every eighth unit count."""
    seen = set()
    units = UNITS if cus == 256 else UNITS[::8] + UNITS[-1:]
    for some in (NS[i:i + 64] for i in range(0, len(NS), 64)):
        cases = [(N, u, s, cus) for N in some for u in units for s in STEPS]
        seen |= _check(cases, planner(cases))
    assert seen == {(nt, ks) for nt in (1, 2, 4) for ks in (1, 2, 4)}, sorted(seen)       # the sweep reaches every plan
    for steps, ks in ((1, 4), (5, 4), (9, 4), (17, 4), (3, 2), (7, 1)):
        sh = M.shares(steps, ks)
        assert sum(sh) == steps and len(sh) == ks and sh == sorted(sh, reverse=True) and sh[0] == -(-steps // ks)


def test_plan_refuses_empty_calls_and_states_its_examples(planner):
    bad = [(0, 16, 1, 256), (-5, 16, 1, 256), (1, 15, 1, 256), (1, 0, 1, 256), (1, 16, 0, 256), (1, 16, -1, 256), (1, 16, 1, 0)]
    assert planner(bad) == [None] * len(bad) and all(M.plan(*c) is None for c in bad)
    # the examples of the header's comment
    got = planner([(64, 1024, 16, 256), (4096, 1024, 1, 256), (4096, 1024, 128, 256)])
    assert got[0][:2] == (1, 4) and got[0][3] == 256                                     # one workgroup per CU
    assert got[1][:2] == (4, 1) and got[2][:2] == (4, 1)
    # the widest grid the sweep's sizes reach stays far below 2^31; so does the largest call the route lets through
    big = [(2 ** 20, 2064, 1024, 256), (2 ** 31 - 1, 16, 1, 256), (2 ** 27, 2 ** 30, 1, 256)]
    for case, got in zip(big, planner(big)):
        assert got == M.plan(*case), case
        assert got is None or got[3] < 2 ** 31


def test_case_table_plans_are_the_header_s(planner):
    cs = M.cases()
    cases = [(c["N"], c["units"], c["K"] // 64, 256) for c in cs]
    for c, case, got in zip(cs, cases, planner(cases)):
        assert got == M.case_plan(c), c["id"]
