"""The cell-range rules and the path choice of the engine (versalignlib_amd/csrc/cell_rules.h) on the CPU: tests/cell_rules_check.cpp
includes that header alone and is built with plain g++ -- no HIP, no GPU -- so every rule that keeps a result exact is
exercised where the suite runs without a device; `tools/sanitize.sh` runs the same program under UBSan."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cell_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def test_cell_rules_check(tmp_path):
    exe = str(tmp_path / "cell_rules_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "cell rules ok" in res.stdout, res.stdout[-3000:]


def test_engine_uses_the_checked_rules():
    """The engine units must run THESE rules: no member copy of one, and no exception used to ask a rule a question."""
    for header in ("cell_rules.h", "cell_constants.h", "align_parts.h", "strip_plan.h", "band_window.h"):
        assert "#include <hip" not in open(os.path.join(CSRC, header)).read(), header
    assert '#include "cell_rules.h"' in open(os.path.join(CSRC, "engine.hip.h")).read()
    for unit in ("engine.hip.h", "engine_core.hip", "engine_score.hip", "engine_long.hip", "engine_align.hip"):
        text = open(os.path.join(CSRC, unit)).read()
        for rule in ("half_float_exact", "half_float_unit_exact", "nw_tilt_span", "tagged_range_ok", "affine_tagged_range_ok",
                     "int16_range_ok", "border_bad", "fill_choice", "score_gap_form"):
            assert "Engine::" + rule not in text and "bool " + rule + "(" not in text, (unit, rule)
        assert "catch (const std::runtime_error" not in text, unit
