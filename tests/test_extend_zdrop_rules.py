"""The extend_zdrop key's rule on the CPU (versalignlib_amd/csrc/extend_zdrop.h: extend_zdrop_choice, extend_zdrop_align_choice,
extend_zdrop_step, extend_zdrop_combine, extend_zdrop_strip_skipped): every branch of the two choices with the key on and off, the
step function against a direct 64-bit restatement, the combine's associativity, scan + predicate against the serial loop, and the
skip condition.  tests/extend_zdrop_rules_check.cpp includes the header alone and is built with plain g++ -- no HIP, no GPU -- and
a second time with -fsanitize=address,undefined: a stand-alone binary, nothing preloaded.  Then where the rule lives: in the
header alone."""
import os
import re
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "extend_zdrop_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + ["-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "extend zdrop rules ok" in res.stdout, res.stdout[-3000:]
    assert "runtime error" not in res.stdout and "AddressSanitizer" not in res.stdout, res.stdout[-3000:]


def test_extend_zdrop_rules_check(tmp_path):
    _build_and_run(tmp_path, "extend_zdrop_rules_check", [])


def test_extend_zdrop_rules_check_under_asan_and_ubsan(tmp_path):
    _build_and_run(tmp_path, "extend_zdrop_rules_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_the_rule_lives_in_its_header_alone():
    rule = open(os.path.join(CSRC, "extend_zdrop.h")).read()
    assert re.findall(r"#include\s+(\S+)", rule) == ['"cell_rules.h"']                      # integers only: no HIP header
    for fn in ("extend_zdrop_step", "extend_zdrop_combine", "extend_zdrop_strip_skipped", "extend_zdrop_unreached", "extend_zdrop_price"):
        assert len(re.findall(r"__host__ __device__ inline \w+ %s\s*\(" % fn, rule)) == 1, fn
    assert len(re.findall(r"\binline\s+PlacedChoice\s+extend_zdrop_choice\s*\(", rule)) == 1
    assert len(re.findall(r"\binline\s+ExtendAlignChoice\s+extend_zdrop_align_choice\s*\(", rule)) == 1
    # Z travels as its own argument: PlacedFacts ends as it did
    rules = open(os.path.join(CSRC, "cell_rules.h")).read()
    facts = rules[rules.index("struct PlacedFacts"):rules.index("struct PlacedChoice")]
    assert re.findall(r"\b(?:bool|int)\s+(\w+)\s*=", facts)[-2:] == ["extend_band", "extend_band_align"] and "zdrop" not in rules
    # the kernel reads the header's functions; no unit restates a refusal's text or the drop arithmetic
    kernel = open(os.path.join(CSRC, "extend_wide_kernels.hip.h")).read()
    for fn in ("extend_zdrop_step(", "extend_zdrop_combine(", "extend_zdrop_strip_skipped(", "extend_zdrop_unreached(", "extend_zdrop_price("):
        assert fn in kernel, fn
    assert "bool ZDROP = false>" in kernel and kernel.count("if constexpr (ZDROP)") >= 2
    for unit in ("engine.hip.h", "engine_core.hip", "engine_placed.hip", "engine_extend.hip", "engine_extend_align.hip", "hip_plugin.hip", "extend_wide_kernels.hip.h",
                 "extend_band_align_kernels.hip.h"):
        text = open(os.path.join(CSRC, unit)).read()
        assert "extend_zdrop: " not in text and "extend_zdrop must" not in text and "price_ref :" not in text, unit
        assert not re.search(r"\binline\s+\w[\w ]*\s+extend_zdrop_(choice|align_choice|step|combine)\s*\(", text), unit
    engine = open(os.path.join(CSRC, "engine_extend.hip")).read()
    assert "extend_zdrop_choice(" in engine and "score_placed_strips(extend_wide_sweep(" in engine and "plan.strips" not in engine
    assert "extend_zdrop_align_choice(" in open(os.path.join(CSRC, "engine_extend_align.hip")).read()
    # the stand-alone program is part of `make sanitize`
    assert "extend_zdrop_rules_check.cpp" in open(os.path.join(ROOT, "tools", "sanitize.sh")).read()
