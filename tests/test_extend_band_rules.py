"""The extend_band key's rule and plan on the CPU (versalignlib_amd/csrc/cell_rules.h: extend_choice, extend_align_choice,
extend_band_int32_ok; extend_band_plan.h: the band's windows): every branch of the two choices with the key on and off, the int32
bound at its edges, and the window functions against a direct enumeration.  tests/extend_band_rules_check.cpp includes the two
headers alone and is built with plain g++ -- no HIP, no GPU -- and a second time with -fsanitize=address,undefined: a stand-alone
binary, nothing preloaded.  Then where the arithmetic lives: in the plan header alone."""
import os
import re
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "extend_band_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + ["-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "extend band rules ok" in res.stdout, res.stdout[-3000:]
    assert "runtime error" not in res.stdout and "AddressSanitizer" not in res.stdout, res.stdout[-3000:]


def test_extend_band_rules_check(tmp_path):
    _build_and_run(tmp_path, "extend_band_rules_check", [])


def test_extend_band_rules_check_under_asan_and_ubsan(tmp_path):
    _build_and_run(tmp_path, "extend_band_rules_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_the_rule_and_the_plan_live_in_their_headers_alone():
    rules = open(os.path.join(CSRC, "cell_rules.h")).read()
    plan = open(os.path.join(CSRC, "extend_band_plan.h")).read()
    assert len(re.findall(r"\binline\s+bool\s+extend_band_int32_ok\s*\(", rules)) == 1
    facts = rules[rules.index("struct PlacedFacts"):rules.index("struct PlacedChoice")]
    members = [line.strip() for line in facts.splitlines() if re.match(r"\s*(bool|int)\s+\w+", line)]
    assert re.match(r"bool extend_band\s*=\s*false;", members[-1]), members[-1]            # trailing, false by default
    assert re.findall(r"#include\s+(\S+)", plan) == ['"../../include/valign_hip.h"']        # integers only: no HIP header
    for fn in ("extend_band_lo", "extend_band_hi", "extend_band_strip", "extend_band_unreached", "extend_band_top_hi", "extend_band_border_col_present",
               "extend_band_border_row_present", "extend_band_half"):
        assert len(re.findall(r"__host__ __device__ inline \w+ %s\s*\(" % fn, plan)) == 1, fn
    # the engine and the kernel read the plan's functions; neither restates the arithmetic or the refusals' texts
    kernel = open(os.path.join(CSRC, "extend_wide_kernels.hip.h")).read()
    engine = open(os.path.join(CSRC, "engine_extend.hip")).read()
    for fn in ("extend_band_strip(", "extend_band_lo(", "extend_band_hi(", "extend_band_border_col_present(", "extend_band_top_hi(", "extend_band_unreached("):
        assert fn in kernel, fn
    assert "extend_band_half(" in engine and not re.search(r"band_width\w*\s*/\s*2", engine)
    for unit in ("engine.hip.h", "engine_core.hip", "engine_placed.hip", "engine_extend.hip", "engine_extend_align.hip", "hip_plugin.hip", "extend_wide_kernels.hip.h"):
        text = open(os.path.join(CSRC, unit)).read()
        assert "extend_band: " not in text and "not built under a band" not in text, unit
    # one strip loop for every pointer-free sweep, the banded one included
    assert "score_placed_strips(extend_wide_sweep(" in engine and "plan.strips" not in engine
