"""The band_nw rules of versalignlib_amd/csrc/cell_rules.h on the CPU: where the banded NW variant may keep the packed int16
strips (band_nw_int16_ok, at its edge), which bands are refused, and the route table with the key off and on.
tests/band_nw_rules_check.cpp includes that header alone and is built with plain g++ -- no HIP, no GPU."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "band_nw_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def test_band_nw_rules_check(tmp_path):
    exe = str(tmp_path / "band_nw_rules_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "band_nw rules ok" in res.stdout, res.stdout[-3000:]


def test_engine_uses_the_checked_rules():
    for unit in ("engine.hip.h", "engine_core.hip", "engine_score.hip", "engine_long.hip", "engine_align.hip"):
        text = open(os.path.join(CSRC, unit)).read()
        for rule in ("band_nw_int16_ok", "band_nw_connects", "band_nw_check"):
            assert "Engine::" + rule not in text and "bool " + rule + "(" not in text, (unit, rule)
    # (the score path's refusals are thrown where its route is decoded: long_plan.h, which engine_long.hip asks)
    assert "band_nw_check(" in open(os.path.join(CSRC, "long_plan.h")).read()
    assert "long_mode(alg, true)" in open(os.path.join(CSRC, "engine_long.hip")).read()
