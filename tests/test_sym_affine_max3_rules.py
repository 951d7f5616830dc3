"""The rule that picks the biased three-operand-maximum form of the int16 symmetric affine Smith-Waterman sweep
(versalignlib_amd/csrc/cell_rules.h: sym_affine_bias, sym_affine_max3_ok) on the CPU: tests/sym_affine_max3_rules_check.cpp
includes that header alone and is built with plain g++ -- no HIP, no GPU.  It also walks the window of bit patterns the form
relies on: all 31,744 positive normal half floats are ordered as their patterns are."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "sym_affine_max3_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def test_sym_affine_max3_rules_check(tmp_path):
    exe = str(tmp_path / "sym_affine_max3_rules_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "sym affine max3 rules ok" in res.stdout, res.stdout[-3000:]


def test_the_engine_asks_the_checked_rule():
    """launch_score takes the form and the bias from cell_rules.h, and the kernel takes the bias from its arguments."""
    text = open(os.path.join(CSRC, "engine_score.hip")).read()
    assert "sym_affine_max3_ok(rule_inputs()" in text and "sym_affine_bias(sc_)" in text
    for unit in ("engine.hip.h", "engine_core.hip", "engine_score.hip"):
        body = open(os.path.join(CSRC, unit)).read()
        assert "Engine::sym_affine_max3_ok" not in body and "bool sym_affine_max3_ok(" not in body, unit
    assert "args.sym_max3_bias" in open(os.path.join(CSRC, "dp_kernels.hip.h")).read()
