"""The rule that hands out the 8 x 19 side tile (versalignlib_amd/csrc/cell_rules.h: sym_affine_side_tile_refusal) on the CPU:
tests/sym_affine_side_tile_rules_check.cpp includes that header alone and is built with plain g++ -- no HIP, no GPU -- once
as it is and once with -fsanitize=address,undefined, each run as its own binary."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "sym_affine_side_tile_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


@pytest.mark.parametrize("flags", ((), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")), ids=("plain", "sanitized"))
def test_sym_affine_side_tile_rules_check(tmp_path, flags):
    exe = str(tmp_path / "sym_affine_side_tile_rules_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, *flags, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "sym affine side tile rules ok" in res.stdout, res.stdout[-3000:]


def test_the_debug_word_is_a_known_one():
    header = open(os.path.join(CSRC, "engine.hip.h")).read()
    assert '"no_side_tile"' in header
