"""The rule that picks the row tables of the tilted int16 symmetric affine Smith-Waterman sweep (versalignlib_amd/csrc/
cell_rules.h: sym_affine_row_tables_ok) on the CPU: tests/sym_affine_row_tables_rules_check.cpp includes that header alone and
is built with plain g++ -- no HIP, no GPU."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "sym_affine_row_tables_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def test_sym_affine_row_tables_rules_check(tmp_path):
    exe = str(tmp_path / "sym_affine_row_tables_rules_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "sym affine row tables rules ok" in res.stdout, res.stdout[-3000:]


def test_the_engine_asks_the_checked_rule():
    """launch_score asks cell_rules.h, sizes the wave's LDS for the path it takes, and the switch is a known one."""
    text = open(os.path.join(CSRC, "engine_score.hip")).read()
    assert "sym_affine_row_tables_ok(rule_inputs()" in text and "row_table_lds(" in text
    assert "a.wave_lds = tables_lds.total" in text and "a.wave_lds * plan.waves_per_block" in text
    header = open(os.path.join(CSRC, "engine.hip.h")).read()
    assert '"no_row_tables"' in header and "in.no_row_tables = no_row_tables_" in header
