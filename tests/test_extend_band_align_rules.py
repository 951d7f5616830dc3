"""extend_align_choice under the extend_band_align key (versalignlib_amd/csrc/cell_rules.h) on the CPU: over the key x the band x
extend_band x score_width x the range, the key off answers exactly as before the key existed (routes, texts, blocks and bytes),
the key on answers Band with the plan's pointer bytes or the stated refusals.  tests/extend_band_align_rules_check.cpp includes the
header alone and is built with plain g++ and a second time with -fsanitize=address,undefined: a stand-alone binary, nothing
preloaded."""
import os
import re
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "extend_band_align_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + ["-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "extend band align rules ok" in res.stdout, res.stdout[-3000:]
    assert "runtime error" not in res.stdout and "AddressSanitizer" not in res.stdout, res.stdout[-3000:]


def test_rules_check(tmp_path):
    _build_and_run(tmp_path, "extend_band_align_rules_check", [])


def test_rules_check_under_asan_and_ubsan(tmp_path):
    _build_and_run(tmp_path, "extend_band_align_rules_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_the_key_is_a_trailing_fact_and_the_engine_asks_the_rule():
    rules = open(os.path.join(CSRC, "cell_rules.h")).read()
    facts = rules[rules.index("struct PlacedFacts"):rules.index("struct PlacedChoice")]
    members = re.findall(r"\b(?:bool|int)\s+(\w+)\s*=", facts)
    assert members[-2:] == ["extend_band", "extend_band_align"] and re.search(r"bool\s+extend_band_align\s*=\s*false\s*;", facts)
    assert len(re.findall(r"\binline\s+ExtendAlignChoice\s+extend_band_align_choice\s*\(", rules)) == 1
    unit = open(os.path.join(CSRC, "engine_extend_align.hip")).read()
    assert "kPlacedRouteBand" in unit and "choice.band_half" in unit and "choice.wave_ptr_bytes" in unit
    # the unit restates neither the band's arithmetic nor a refusal's text
    assert not re.search(r"band_width\w*\s*/\s*2", unit) and "extend_band: " not in unit and "extend_band_align must" not in unit
    placed = open(os.path.join(CSRC, "engine_placed.hip")).read()
    assert re.search(r"extend_band_,\s*extend_band_align_\}", placed)                        # placed_facts carries the key, last
