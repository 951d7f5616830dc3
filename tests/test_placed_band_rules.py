"""placed_choice under band_placed (versalignlib_amd/csrc/cell_rules.h, with the chain's plan of long_plan.h) on the CPU: the
key off and on, with and without a band, every refusal, and the range rules at their edges.  tests/placed_band_rules_check.cpp
includes the pure headers and is built with plain g++ -- no HIP, no GPU.  Then the binding: the setter is exported, declared
and bound, and the public header states the definition."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT
from versalignlib_amd import build as b
from versalignlib_amd import hipkernel

SRC = os.path.join(ROOT, "tests", "placed_band_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "valign_hip.h")


def test_placed_band_rules_check(tmp_path):
    exe = str(tmp_path / "placed_band_rules_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "placed band rules ok" in res.stdout, res.stdout[-3000:]


def test_the_rule_lives_in_the_header_and_the_kernel_is_instantiated_once():
    rules = open(os.path.join(CSRC, "cell_rules.h")).read()
    assert re.search(r"inline\s+bool\s+band_placed_key_ok\s*\(", rules) and "kBandPlacedKeyBits" in rules
    placed = open(os.path.join(CSRC, "engine_placed.hip")).read()
    assert "band_placed_key_ok" not in placed and "kBandPlacedKeyBits" not in placed          # the engine asks placed_choice
    assert "PlacedRoute::Chain" in placed and "score_band_device(" in placed and "hipOccupancyMaxActiveBlocksPerMultiprocessor" not in placed
    # the PLACED form is named with its template arguments in one place: the lookup beside band_kernel()
    hits = []
    for name in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, name)).read()
        hits += [name] * len(re.findall(r"score_band_kernel<[^>;]*,\s*false,\s*true>", text))
    assert hits == ["engine_long.hip"], hits
    assert "placed_band_rules_check.cpp" in open(os.path.join(ROOT, "tools", "sanitize.sh")).read()


def test_setter_is_exported_declared_and_bound():
    if not os.path.exists(b.HIP_PLUGIN):
        b.build_hip()
    assert hasattr(ctypes.CDLL(b.HIP_PLUGIN), "valign_hip_set_band_placed")
    assert "valign_hip_set_band_placed" in hipkernel.EXPORTED_SYMBOLS
    assert callable(getattr(hipkernel.Engine, "set_band_placed"))
    L = hipkernel.lib()
    assert L.valign_hip_set_band_placed.argtypes == [ctypes.c_void_p, ctypes.c_int]
    # without an engine every value is refused with a message, and without a device (values 2 and -1 on an engine: the GPU suite)
    for value in (0, 1, 2, -1):
        assert L.valign_hip_set_band_placed(None, value) != 0
        assert b"null engine" in L.valign_hip_last_error()
    text = open(HEADER).read()
    assert re.search(r"\bint\s+valign_hip_set_band_placed\s*\(\s*valign_hip_engine\s*\*\s*e\s*,\s*int\s+on\s*\)\s*;", text)
    for phrase in ("band_width > 0", "band_placed", "first IN-BAND cell", "{0, 0, 0}", "2 * max(R, F)", "band_block_rows", '"chain"', "no fall-back"):
        assert phrase in text, phrase
