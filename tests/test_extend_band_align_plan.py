"""The pointer layout of banded extension alignments (versalignlib_amd/csrc/extend_band_align_plan.h) on the CPU:
tests/extend_band_align_plan_check.cpp includes the plan header alone and compares it with a direct enumeration -- every present
cell of every strip in bounds, no two cells on the same bits, block counts at step counts = 0, 1, 7 (mod 8), no block for an empty
strip, the totals of shapes of one to four strips at w from 0 to the limit.  Built with g++ -fsanitize=address,undefined and run as
its own program: nothing is preloaded, no HIP, no GPU.  Then who states the layout: the header alone."""
import os
import re
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "extend_band_align_plan_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def test_plan_check_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "extend_band_align_plan_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC, SRC,
                            "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "extend band align plan ok" in res.stdout, res.stdout[-3000:]
    assert "runtime error" not in res.stdout and "AddressSanitizer" not in res.stdout, res.stdout[-3000:]


def test_the_layout_lives_in_the_plan_header_alone():
    plan = open(os.path.join(CSRC, "extend_band_align_plan.h")).read()
    assert re.findall(r"#include\s+(\S+)", plan) == ['"extend_band_plan.h"']                # integers only: no HIP header
    for fn in ("extend_band_align_strip_blocks", "extend_band_align_strip_base", "extend_band_align_pp_dwords", "extend_band_align_word",
               "extend_band_align_shift", "extend_band_align_slot"):
        assert len(re.findall(r"__host__ __device__ inline [\w ]+ %s\s*\(" % fn, plan)) == 1, fn
    sweep = open(os.path.join(CSRC, "extend_wide_kernels.hip.h")).read()
    kernels = open(os.path.join(CSRC, "extend_band_align_kernels.hip.h")).read()
    rules = open(os.path.join(CSRC, "cell_rules.h")).read()
    # the fill, the walk and the rule read the plan's functions
    for fn in ("extend_band_align_pp_dwords(", "extend_band_align_strip_base(", "extend_band_align_word("):
        assert fn in sweep, fn
    for fn in ("extend_band_align_strip_base(", "extend_band_align_word(", "extend_band_strip("):
        assert fn in kernels, fn
    assert "extend_band_align_pp_dwords(" in rules and "extend_band_align_blocks_before(" in rules
    # vector stores in plain C++: no inline assembly in the pointer stream's code
    assert "asm" not in kernels
