"""The plan of the row-strip alignment path (versalignlib_amd/csrc/strip_plan.h: the strip mode, the compiled instances, rows per
lane, what a pair-of-pairs holds in the scratch and where) on the CPU: tests/strip_plan_check.cpp includes the pure headers and is
built with plain g++ -- no HIP, no GPU."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "strip_plan_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def test_strip_plan_check(tmp_path):
    exe = str(tmp_path / "strip_plan_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "strip plan ok" in res.stdout, res.stdout[-3000:]


def test_the_engine_has_one_plan_and_one_lookup():
    """The strip path decodes the route, sizes its scratch and picks its kernel through the checked header alone."""
    text = open(os.path.join(CSRC, "engine_align.hip")).read()
    for name in ("strip_mode(", "strip_rows_per_lane(", "strip_plan(", "strip_scratch_cap(", "strip_instance_exists("):
        assert name in text, name
    for gone in ("VALIGN_STRIP_", "the plan and the strips disagree", "bool wide, bool band, bool ckpt"):
        assert gone not in text, gone
