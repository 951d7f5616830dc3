"""placed_choice and span_choice under placed_wide (versalignlib_amd/csrc/cell_rules.h) on the CPU: the key off changes nothing,
the key on gives Wide exactly where the two int16 refusals applied, each range rule at its edge.
tests/placed_wide_rules_check.cpp includes the pure header and is built here with g++ -fsanitize=address,undefined as a
stand-alone program -- no HIP, no GPU.  Then the binding: the setter is exported, declared and bound, the public header
states the definition, and a null engine is refused."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT
from versalignlib_amd import build as b
from versalignlib_amd import hipkernel

SRC = os.path.join(ROOT, "tests", "placed_wide_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "valign_hip.h")


def test_placed_wide_rules_check(tmp_path):
    exe = str(tmp_path / "placed_wide_rules_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "placed wide rules ok" in res.stdout, res.stdout[-3000:]


def test_the_rule_lives_in_the_header_and_the_kernel_in_the_placed_unit():
    rules = open(os.path.join(CSRC, "cell_rules.h")).read()
    assert re.search(r"enum\s+class\s+PlacedRoute\s*\{[^}]*Chain\s*,\s*Wide\s*\}", rules)              # appended at the end
    assert re.search(r"bool\s+placed_wide\s*=\s*false\s*;[^}]*\}\s*;\s*\n\s*\nstruct\s+PlacedChoice", rules)      # the last member of PlacedFacts
    placed = open(os.path.join(CSRC, "engine_placed.hip")).read()
    assert '#include "placed_wide_kernels.hip.h"' in placed and "PlacedRoute::Wide" in placed and "score_placed_wide_kernel<" in placed
    assert "int32_refused" not in placed and "int16_range_ok" not in placed                           # the engine asks placed_choice
    assert "placed_wide_kernels.hip.h" in b.HIP_HEADERS and "engine_placed.hip" in b.HIP_SOURCES       # no new translation unit
    kernel = open(os.path.join(CSRC, "placed_wide_kernels.hip.h")).read()
    assert "strip_ring_setup<K>" in kernel and "fetch_profile<" in kernel and "first_bad" not in kernel.split("#pragma once")[1]
    # not a StripMode{wide, ckpt} instance: the strip table stays as tests/strip_plan_check.cpp pins it
    assert "m.ckpt && (m.sse || m.band || m.wide)" in open(os.path.join(CSRC, "strip_plan.h")).read()
    for name in sorted(os.listdir(CSRC)):
        if name != "engine_placed.hip":
            assert "score_placed_wide_kernel<" not in open(os.path.join(CSRC, name)).read(), name


def test_setter_is_exported_declared_and_bound():
    if not os.path.exists(b.HIP_PLUGIN):
        b.build_hip()
    assert hasattr(ctypes.CDLL(b.HIP_PLUGIN), "valign_hip_set_placed_wide")
    assert "valign_hip_set_placed_wide" in hipkernel.EXPORTED_SYMBOLS
    assert callable(getattr(hipkernel.Engine, "set_placed_wide"))
    L = hipkernel.lib()
    assert L.valign_hip_set_placed_wide.argtypes == [ctypes.c_void_p, ctypes.c_int]
    # without an engine every value is refused with a message, and without a device (values 2 and -1 on an engine: the GPU suite)
    for value in (0, 1, 2, -1):
        assert L.valign_hip_set_placed_wide(None, value) != 0
        assert b"null engine" in L.valign_hip_last_error()


def test_header_declares_it_and_states_the_definition():
    text = open(HEADER).read()
    assert re.search(r"\bint\s+valign_hip_set_placed_wide\s*\(\s*valign_hip_engine\s*\*\s*e\s*,\s*int\s+on\s*\)\s*;", text)
    flat = " ".join(" ".join(re.sub(r"^\s*/?\*+\s?", "", line) for line in text.splitlines()).split())      # comment text, line frames removed
    for phrase in ("key placed_wide", "score_width = 32", "unless valign_hip_set_placed_wide(e, 1) asks for them, below", "does NOT saturate at 32767",
                   "DefaultKernel.cpp:252-256", "{0, 0, 0}", "five zeros", "WHAT THE KEY DOES NOT CHANGE", "int16 or refuse", "not read under a band",
                   '"placed_wide:"', "(R + F + 2) x |score| >= 2^28", '"ran_placed": "wide"', '"wide/wide"', "Other values than 0 / 1 are refused"):
        assert phrase in flat, phrase
    # the lines the earlier binding tests look for are still there
    for phrase in ("band_width > 0", "traceback_policy = 1", "opt & 0xF == 1", "WHATEVER band_placed says"):
        assert phrase in flat, phrase
