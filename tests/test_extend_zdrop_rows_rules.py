"""The extend_zdrop_rows key's rule on the CPU (versalignlib_amd/csrc/extend_zdrop.h: extend_zdrop_replay_lane, extend_zdrop_lane_best,
extend_zdrop_record_lane, extend_zdrop_rows_choice, extend_zdrop_rows_align_choice): the lane form of the drop rule -- G lanes of K
rows, local combine, exclusive scan, replay, minimum -- against the serial loop on the six full geometries, and every branch of the
two choices with the key on and off.  tests/extend_zdrop_rows_rules_check.cpp includes the header alone and is built with plain g++
-- no HIP, no GPU -- and a second time with -fsanitize=address,undefined: a stand-alone binary, nothing preloaded.  Then where the
rule lives: in the header alone, shared by the two kernels through one device function."""
import os
import re
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "extend_zdrop_rows_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + ["-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "extend zdrop rows rules ok" in res.stdout, res.stdout[-3000:]
    assert "runtime error" not in res.stdout and "AddressSanitizer" not in res.stdout, res.stdout[-3000:]


def test_extend_zdrop_rows_rules_check(tmp_path):
    _build_and_run(tmp_path, "extend_zdrop_rows_rules_check", [])


def test_extend_zdrop_rows_rules_check_under_asan_and_ubsan(tmp_path):
    _build_and_run(tmp_path, "extend_zdrop_rows_rules_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_the_lane_form_lives_in_the_header_and_one_device_function():
    rule = open(os.path.join(CSRC, "extend_zdrop.h")).read()
    for fn in ("extend_zdrop_replay_lane", "extend_zdrop_lane_best", "extend_zdrop_record_lane"):
        assert len(re.findall(r"__host__ __device__ inline \w+ %s\s*\(" % fn, rule)) == 1, fn
    assert len(re.findall(r"\binline\s+PlacedChoice\s+extend_zdrop_rows_choice\s*\(", rule)) == 1
    assert len(re.findall(r"\binline\s+ExtendAlignChoice\s+extend_zdrop_rows_align_choice\s*\(", rule)) == 1
    assert "the int32 route of unbanded extension alignments has no Z-drop form" in rule
    # the header states why the minimum of the lanes' answers is the serial drop row
    assert "Why the minimum is the serial rule's T" in rule and "all greater than T" in rule
    # one device function, shared by the two kernels; the step loops do not know the key
    scores = open(os.path.join(CSRC, "extend_kernels.hip.h")).read()
    fills = open(os.path.join(CSRC, "extend_align_kernels.hip.h")).read()
    assert len(re.findall(r"__device__ __forceinline__ ExtendRec extend_zdrop_rows_record\s*\(", scores)) == 1
    assert scores.count("extend_zdrop_rows_record<G, K>(") == 1 and fills.count("extend_zdrop_rows_record<G, K>(") == 1
    assert "template <int G, int K, int GAPS, bool ZDROP = false>" in scores and "template <int G, int K, bool AFFINE, bool ZDROP = false>" in fills
    for text in (scores, fills):
        step = text[text.index("auto step = [&]"):text.index("const int steps =")]
        assert "ZDROP" not in step and "zdrop" not in step
        assert text.count("if constexpr (ZDROP)") == 1
    for fn in ("extend_zdrop_replay_lane(", "extend_zdrop_lane_best(", "extend_zdrop_combine(", "extend_zdrop_record_lane(", "extend_zdrop_unreached("):
        assert fn in scores, fn
    # the engine asks the new choices; no unit restates a text
    assert "extend_zdrop_rows_choice(" in open(os.path.join(CSRC, "engine_extend.hip")).read()
    assert "extend_zdrop_rows_align_choice(" in open(os.path.join(CSRC, "engine_extend_align.hip")).read()
    for unit in ("engine.hip.h", "engine_core.hip", "engine_extend.hip", "engine_extend_align.hip", "hip_plugin.hip", "extend_kernels.hip.h", "extend_align_kernels.hip.h"):
        text = open(os.path.join(CSRC, unit)).read()
        assert "extend_zdrop: " not in text and "extend_zdrop_rows must" not in text, unit
    # the stand-alone program is part of `make sanitize`
    assert "extend_zdrop_rows_rules_check.cpp" in open(os.path.join(ROOT, "tools", "sanitize.sh")).read()
