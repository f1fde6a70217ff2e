"""The plan of the byte first layer's image-wide strip (csrc/qnn_first_u8.hip, W = 32): one strip per row.  At the
benchmark's batch every resident wave gets exactly one whole image.  No GPU; the planner is compiled as in
tests/test_strip_plan.py."""
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
    StripPlan p;
    if (!qnn_strip_plan(&p, 4096, 1, 16, 1024, 1.5, 2)) return 1;
    printf("%d %d %d %d %u\n", p.spr, p.rc, p.nch, p.ntasks, p.blocks);
    return 0;
}
"""


def test_one_task_per_resident_wave_at_the_benchmark_batch(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src, exe = tmp_path / "plan_wide.cpp", tmp_path / "plan_wide"
    src.write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [1, 16, 1, 4096, 1024]               # spr, rc, nch, tasks, workgroups
