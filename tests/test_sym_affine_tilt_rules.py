"""The rule that picks the tilted frame of the biased int16 symmetric affine Smith-Waterman sweep
(versalignlib_amd/csrc/cell_rules.h: sym_affine_tilt_bias, sym_affine_tilt_ok) on the CPU: tests/sym_affine_tilt_rules_check.cpp
includes that header alone and is built with plain g++ -- no HIP, no GPU."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "sym_affine_tilt_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def test_sym_affine_tilt_rules_check(tmp_path):
    exe = str(tmp_path / "sym_affine_tilt_rules_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "sym affine tilt rules ok" in res.stdout, res.stdout[-3000:]


def test_the_engine_asks_the_checked_rule():
    """launch_score takes the frame and its bias from cell_rules.h beside the plain form's, and the switch is a known one."""
    text = open(os.path.join(CSRC, "engine_score.hip")).read()
    assert "sym_affine_tilt_ok(rule_inputs()" in text and "sym_affine_tilt_bias(sc_)" in text
    assert "sym_affine_max3_ok(rule_inputs()" in text and "sym_affine_bias(sc_)" in text
    header = open(os.path.join(CSRC, "engine.hip.h")).read()
    assert '"no_tilt"' in header and "no_max3_, no_tilt_}" in header
    for unit in ("engine.hip.h", "engine_core.hip", "engine_score.hip"):
        body = open(os.path.join(CSRC, unit)).read()
        assert "Engine::sym_affine_tilt_ok" not in body and "bool sym_affine_tilt_ok(" not in body, unit
