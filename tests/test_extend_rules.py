"""extend_choice of versalignlib_amd/csrc/cell_rules.h on the CPU: every refusal of an extension-score call and both sides of each
edge of its signed int16 bound.  tests/extend_rules_check.cpp includes that header alone and is built with plain g++ -- no HIP,
no GPU -- and a second time with -fsanitize=address,undefined: a stand-alone binary, nothing preloaded."""
import os
import re
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "extend_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + ["-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "extend rules ok" in res.stdout, res.stdout[-3000:]
    assert "runtime error" not in res.stdout and "AddressSanitizer" not in res.stdout, res.stdout[-3000:]


def test_extend_rules_check(tmp_path):
    _build_and_run(tmp_path, "extend_rules_check", [])


def test_extend_rules_check_under_asan_and_ubsan(tmp_path):
    _build_and_run(tmp_path, "extend_rules_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_engine_asks_the_rule_and_holds_no_copy():
    units = ("engine.hip.h", "engine_core.hip", "engine_score.hip", "engine_placed.hip", "engine_subopt.hip", "engine_extend.hip", "hip_plugin.hip",
             "extend_kernels.hip.h")
    for unit in units:
        text = open(os.path.join(CSRC, unit)).read()
        assert "Engine::extend_choice" not in text and not re.search(r"\b(inline|constexpr|PlacedChoice)\s+extend_choice\s*\(", text), unit
        for phrase in ("opt & 0xF == 0 only", "not built for band_width", "not built for score_width", "register sweep only", "signed int16 cells: shape"):
            assert phrase not in text, (unit, phrase)          # (the refusals' texts live in the header)
        assert not re.search(r"\binline\s+\w[\w ]*\s+extend_(int16_ok|cell_top|cell_bottom)\s*\(", text), unit
    rules = open(os.path.join(CSRC, "cell_rules.h")).read()
    assert len(re.findall(r"\binline\s+PlacedChoice\s+extend_choice\s*\(", rules)) == 1
    unit = open(os.path.join(CSRC, "engine_extend.hip")).read()
    assert "extend_choice(" in unit
    # the unit decides nothing about a refusal itself: neither the band, the cell width, the policy nor the read length is tested there
    for word in ("band_width_", "score_width_", "sse_policy_", "kPlacedStripRows", "32000"):
        assert word not in unit, word
