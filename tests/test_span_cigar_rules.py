"""span_cigar_choice of versalignlib_amd/csrc/cell_rules.h on the CPU: every refusal of a spanned CIGAR call and its text, and
the routes of the calls that run.  tests/span_cigar_rules_check.cpp includes that header alone; it is built once with plain g++
and once as a stand-alone program with -fsanitize=address,undefined -- no HIP, no GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "span_cigar_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_span_cigar_rules_check(tmp_path, flags):
    exe = str(tmp_path / "span_cigar_rules_check")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC] + flags + [SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "span cigar rules ok" in res.stdout, res.stdout[-3000:]


def test_engine_asks_the_rule_and_holds_no_copy():
    unit = open(os.path.join(CSRC, "engine_span_cigar.hip")).read()
    assert "span_cigar_choice(" in unit and "Engine::span_cigar_choice" not in unit
    for text in ("spanned CIGARs: \"", "not built for band_width", "Smith-Waterman only"):        # (the refusals' texts live in the header)
        assert text not in unit, text
    # refusals leave before anything is staged or launched: the rule is asked in span_cigar_prepare, which both entry points
    # call before their first allocation, copy or launch
    prepare = unit.split("Engine::span_cigar_prepare", 1)[1].split("Engine::span_cigar_chunk_pairs", 1)[0]
    assert "span_cigar_choice(" in prepare and "hipLaunch" not in prepare and "hipMemcpy" not in prepare
    for entry in ("Engine::align_span_device", "Engine::align_span_host"):
        body = unit.split("void " + entry if "device" in entry else "bool " + entry, 1)[1]
        first = min(body.find(word) for word in ("ensure_", "hipMemcpy", "span_cigar_chunk(") if word in body)
        assert 0 < body.find("span_cigar_prepare(") < first, entry
