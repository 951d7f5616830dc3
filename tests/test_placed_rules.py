"""placed_choice of versalignlib_amd/csrc/cell_rules.h on the CPU: the lane key at its edge, every refusal, the strip threshold
on both sides.  tests/placed_rules_check.cpp includes that header alone and is built with plain g++ -- no HIP, no GPU."""
import os
import re
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "placed_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def test_placed_rules_check(tmp_path):
    exe = str(tmp_path / "placed_rules_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "placed rules ok" in res.stdout, res.stdout[-3000:]


def test_engine_asks_the_rule_and_holds_no_copy():
    units = ("engine.hip.h", "engine_core.hip", "engine_score.hip", "engine_long.hip", "engine_align.hip", "engine_cigar.hip",
             "engine_placed.hip", "hip_plugin.hip", "placed_kernels.hip.h")
    for unit in units:
        text = open(os.path.join(CSRC, unit)).read()
        for rule in ("placed_choice", "placed_key_bits"):
            assert "Engine::" + rule not in text and not re.search(r"\b(inline|constexpr|bool|int|PlacedChoice)\s+" + rule + r"\s*\(", text), (unit, rule)
        assert "32000" not in text or unit != "engine_placed.hip", unit          # (the key's bound lives in the header)
        assert "kPlacedStripRows =" not in text, unit
    placed = open(os.path.join(CSRC, "engine_placed.hip")).read()
    assert "placed_choice(" in placed and "<< " not in placed.split("placed_plan_for", 1)[1].split("score_placed_device", 1)[0]
    # the kernels take the key's bits from the rule's function, and the sanitizer run includes the check
    assert "placed_key_bits(K)" in open(os.path.join(CSRC, "placed_kernels.hip.h")).read()
    assert "placed_rules_check.cpp" in open(os.path.join(ROOT, "tools", "sanitize.sh")).read()
