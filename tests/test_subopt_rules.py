"""subopt_choice of versalignlib_amd/csrc/cell_rules.h on the CPU: every refusal of a suboptimal-score call and both tracks of one
that runs.  tests/subopt_rules_check.cpp includes that header alone and is built with plain g++ -- no HIP, no GPU."""
import os
import re
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "subopt_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def test_subopt_rules_check(tmp_path):
    exe = str(tmp_path / "subopt_rules_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "subopt rules ok" in res.stdout, res.stdout[-3000:]


def test_engine_asks_the_rule_and_holds_no_copy():
    units = ("engine.hip.h", "engine_core.hip", "engine_score.hip", "engine_long.hip", "engine_align.hip", "engine_cigar.hip",
             "engine_placed.hip", "engine_span.hip", "engine_subopt.hip", "hip_plugin.hip", "subopt_kernels.hip.h", "placed_kernels.hip.h")
    for unit in units:
        text = open(os.path.join(CSRC, unit)).read()
        assert "Engine::subopt_choice" not in text and not re.search(r"\b(inline|constexpr|PlacedChoice)\s+subopt_choice\s*\(", text), unit
        for phrase in ("need mask >= 0", "not built for band_width", "register sweep only", "no room for its column ring"):          # (the refusals' texts live in the header)
            assert phrase not in text, (unit, phrase)
        assert not re.search(r"\b(inline|constexpr|int)\s+subopt_block_waves\s*\(", text), unit
    rules = open(os.path.join(CSRC, "cell_rules.h")).read()
    assert len(re.findall(r"\binline\s+PlacedChoice\s+subopt_choice\s*\(", rules)) == 1
    unit = open(os.path.join(CSRC, "engine_subopt.hip")).read()
    assert "subopt_choice(" in unit
    # the unit decides nothing about a route itself: neither the mask's sign, the band nor the read length is tested there
    assert "mask < 0" not in unit and "band_width_" not in unit and "kPlacedStripRows" not in unit
    assert "subopt_rules_check.cpp" in open(os.path.join(ROOT, "tools", "sanitize.sh")).read()
