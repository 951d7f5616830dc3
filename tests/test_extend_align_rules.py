"""extend_align_choice of versalignlib_amd/csrc/cell_rules.h on the CPU: an extension-alignment call is refused exactly where an
extension-score call on the register sweep is, with its texts, and -- with a text of its own -- wherever extend_wide = 1 would move
the scores to the int32 sweep; and the pointer scratch a wave needs.  tests/extend_align_rules_check.cpp includes that header
alone and is built with plain g++ -- no HIP, no GPU -- and a second time with -fsanitize=address,undefined: a stand-alone binary,
nothing preloaded."""
import os
import re
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "extend_align_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + ["-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "extend align rules ok" in res.stdout, res.stdout[-3000:]
    assert "runtime error" not in res.stdout and "AddressSanitizer" not in res.stdout, res.stdout[-3000:]


def test_extend_align_rules_check(tmp_path):
    _build_and_run(tmp_path, "extend_align_rules_check", [])


def test_extend_align_rules_check_under_asan_and_ubsan(tmp_path):
    _build_and_run(tmp_path, "extend_align_rules_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_engine_asks_the_rule_and_holds_no_copy():
    rules = open(os.path.join(CSRC, "cell_rules.h")).read()
    assert len(re.findall(r"\binline\s+ExtendAlignChoice\s+extend_align_choice\s*\(", rules)) == 1
    assert len(re.findall(r"\binline\s+long long\s+extend_align_wave_ptr_bytes\s*\(", rules)) == 1
    unit = open(os.path.join(CSRC, "engine_extend_align.hip")).read()
    assert "extend_align_choice(" in unit and "wave_ptr_bytes" in unit
    # the unit decides nothing about a refusal itself: neither the band, the cell width, the policy nor the read length is tested
    # there, and the refusals' texts live in the header
    for word in ("band_width_", "score_width_", "sse_policy_", "extend_wide_", "kPlacedStripRows", "32000", "extension alignments: not built"):
        assert word not in unit, word
    for other in ("engine.hip.h", "engine_core.hip", "engine_extend.hip", "hip_plugin.hip", "extend_align_kernels.hip.h"):
        text = open(os.path.join(CSRC, other)).read()
        assert not re.search(r"\b(inline|constexpr|ExtendAlignChoice)\s+extend_align_choice\s*\(", text), other
