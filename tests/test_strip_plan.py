"""The host-side task plan of the row-walking kernels (csrc/qnn_strip_plan.h) against an independent statement of its cost
model.  No GPU: the header is plain C++, compiled here into a stand-alone program with the address and undefined-behaviour
sanitizers.

LAUNCHERS below restates the (rc_step, fill) each launcher passes; nothing here reads the .hip files, so that a call site
passes these values is checked by review of the call site, not by this test."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quantizedneuralnetworks-keras-tensorflow_amd", "csrc")

MAIN = r"""
#include <stdio.h>
#include "qnn_strip_plan.h"
int main() {
    int N, spr, rows, cap, step;
    double fill;
    while (scanf("%d %d %d %d %lf %d", &N, &spr, &rows, &cap, &fill, &step) == 6) {
        StripPlan p;
        if (!qnn_strip_plan(&p, N, spr, rows, cap, fill, step)) { printf("refused\n"); continue; }
        printf("%d %d %d %d %u\n", p.spr, p.rc, p.nch, p.ntasks, p.blocks);
    }
    return 0;
}
"""

# launcher: (rc_step, fill), as the launchers pass them; all of them walk `rows` = H, Ho or H/2 of their layer
LAUNCHERS = {
    "launch_strip": (1, 3), "launch_strip_s2": (1, 2), "launch_strip8": (1, 3), "launch_strip8_s2": (1, 2),
    "qnn_launch_strip16_lds": (4, 3), "qnn_try_launch_stem": (1, 2),
    "qnn_try_launch_first_u8": (2, 1.5), "qnn_try_launch_first_fixed": (2, 1.5),
}
ROWS = (1, 2, 3, 4, 5, 7, 8, 9, 10, 16, 28, 32, 56, 112, 224)
SPR = (1, 2, 14)
BATCH = (1, 2, 3, 64, 260, 4096)
CAPS = (64, 128, 256, 512, 768, 1024, 1536)


def ceil_div(a, b):
    return -(-a // b)


def model(N, spr, rows, cap, fill, step):
    """The plan as the launchers' table states it: candidates by step, cost = rounds * (rc + fill), first minimum wins."""
    cands = range(min(rows, 4), rows + 1) if step == 1 else range(step, rows + step, step)
    rc, nch, best = rows, 1, float("inf")
    for c in cands:
        cost = ceil_div(N * spr * ceil_div(rows, c), 4 * cap) * (c + fill)
        if cost < best:
            rc, nch, best = c, ceil_div(rows, c), cost
    ntasks = N * spr * nch
    return None if ntasks >= 2000000000 else (rc, nch, ntasks, min(ceil_div(ntasks, 4), cap))


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("strip_plan")
    src, exe = d / "plan_main.cpp", d / "plan_main"
    src.write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def run(cases):
        text = "".join("%d %d %d %d %r %d\n" % c for c in cases)
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
        out = [ln for ln in out if ln]
        assert len(out) == len(cases)
        return [None if ln == "refused" else tuple(int(v) for v in ln.split()) for ln in out]
    return run


def test_plan_matches_the_cost_model_for_every_launcher(planner):
    cases, names = [], []
    for name, (step, fill) in LAUNCHERS.items():
        for rows, spr, N, cap in itertools.product(ROWS, SPR, BATCH, CAPS):
            cases.append((N, spr, rows, cap, float(fill), step))
            names.append(name)
    got = planner(cases)
    for name, case, g in zip(names, cases, got):
        N, spr, rows, cap, fill, step = case
        assert g is not None, (name, case)
        g_spr, rc, nch, ntasks, blocks = g
        assert g_spr == spr and (rc, nch, ntasks, blocks) == model(*case), (name, case, g, model(*case))
        # the chunks cover the rows with no empty last chunk; the grid is within what is resident and what there is to do
        assert nch * rc >= rows and (nch - 1) * rc < rows, (name, case, g)
        assert 1 <= blocks <= cap and blocks <= ceil_div(ntasks, 4), (name, case, g)
        if step > 1:
            assert rc % step == 0, (name, case, g)


def test_plan_refuses_at_two_billion_tasks(planner):
    below = (1999999999, 1, 1, 1024, 3.0, 1)
    at = (2000000000, 1, 1, 1024, 3.0, 1)
    split = (500000000, 2, 2, 1024, 1.5, 2)          # one chunk of two row pairs: 10^9 tasks
    split_at = (500000000, 4, 2, 1024, 1.5, 2)
    got = planner([below, at, split, split_at])
    assert got[0] == (1, 1, 1, 1999999999, 1024) and model(*below) == (1, 1, 1999999999, 1024)
    assert got[1] is None and model(*at) is None
    assert got[2] == (2, 2, 1, 1000000000, 1024) and model(*split) == (2, 1, 1000000000, 1024)
    assert got[3] is None and model(*split_at) is None


def test_plan_refuses_an_empty_walk(planner):
    """No image, no strip, no row or no resident workgroup: refused before any division (no caller passes these)."""
    ok = (2, 1, 10, 256, 3.0, 1)
    empty = [(0, 1, 10, 256, 3.0, 1), (2, 0, 10, 256, 3.0, 1), (2, 1, 0, 256, 3.0, 1), (2, 1, 0, 256, 1.5, 2), (2, 1, 10, 0, 3.0, 1)]
    got = planner([ok] + empty)
    assert got[0] == (1, 4, 3, 6, 2)
    assert got[1:] == [None] * len(empty)
