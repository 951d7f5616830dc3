"""The plan of the checkpointed traceback (versalignlib_amd/csrc/ckpt_plan.h: scratch bytes per pair-of-pairs, chunks under a
cap, the round list) and its route (cell_rules.h: AlignRoute::StripCkpt) on the CPU: tests/ckpt_plan_check.cpp includes the two
pure headers and is built with plain g++ -- no HIP, no GPU."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "ckpt_plan_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def test_ckpt_plan_check(tmp_path):
    exe = str(tmp_path / "ckpt_plan_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "ckpt plan ok" in res.stdout, res.stdout[-3000:]


def test_the_engine_runs_the_checked_plan():
    """The headers are pure, and the engine sizes its scratch with them rather than with arithmetic of its own: the one plan of
    the strip path (strip_plan.h), of which ckpt_plan() is the checkpointed view."""
    for header in ("ckpt_plan.h", "strip_plan.h"):
        assert "#include <hip" not in open(os.path.join(CSRC, header)).read(), header
    assert "strip_plan(" in open(os.path.join(CSRC, "ckpt_plan.h")).read()
    text = open(os.path.join(CSRC, "engine_align.hip")).read()
    for name in ("strip_plan(", "strip_chunk_pairs(", "ckpt_rounds("):
        assert name in text, name
