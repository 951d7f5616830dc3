"""span_ref_length and span_choice of versalignlib_amd/csrc/cell_rules.h on the CPU: the bound of the reverse sweep at its edges
and every refusal of a spanned call.  tests/span_rules_check.cpp includes that header alone and is built with plain g++ -- no
HIP, no GPU."""
import os
import re
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "span_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def test_span_rules_check(tmp_path):
    exe = str(tmp_path / "span_rules_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "span rules ok" in res.stdout, res.stdout[-3000:]


def test_engine_asks_the_rule_and_holds_no_copy():
    units = ("engine.hip.h", "engine_core.hip", "engine_score.hip", "engine_long.hip", "engine_align.hip", "engine_cigar.hip",
             "engine_placed.hip", "engine_span.hip", "hip_plugin.hip", "span_kernels.hip.h")
    for unit in units:
        text = open(os.path.join(CSRC, unit)).read()
        for rule in ("span_ref_length", "span_choice"):
            assert "Engine::" + rule not in text and not re.search(r"\b(inline|constexpr|long long|int|PlacedChoice)\s+" + rule + r"\s*\(", text), (unit, rule)
        assert "not built for band_width" not in text, unit                  # (the refusals' texts live in the header)
    span = open(os.path.join(CSRC, "engine_span.hip")).read()
    assert "span_choice(" in span and "span_ref_length(" in span
    # no arithmetic of the bound in the unit: nothing divides, and the scoring's gap fields are not read
    prepare = span.split("Engine::span_prepare", 1)[1].split("Engine::span_chunk_pairs", 1)[0]
    assert " / " not in prepare and "gap_read" not in span and "ext_read" not in span and "open_read" not in span
    # the reverse sweep's shape is the rule's value, once, where the child engine is made; describe reports the rule's value
    assert span.count("span_ref_length(") == 1
    assert "span_ref_length(rule_inputs())" in open(os.path.join(CSRC, "engine_core.hip")).read()
    assert "span_rules_check.cpp" in open(os.path.join(ROOT, "tools", "sanitize.sh")).read()
