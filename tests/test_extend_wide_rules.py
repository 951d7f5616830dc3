"""extend_choice under the extend_wide key and extend_int32_ok (versalignlib_amd/csrc/cell_rules.h) on the CPU: with the key off
the rule decides as before the key, with the key on the int32 sweep opens exactly where the rule names it, and both sides of
each edge of the int32 bound.  tests/extend_wide_rules_check.cpp includes that header alone and is built with plain g++ -- no
HIP, no GPU -- and a second time with -fsanitize=address,undefined: a stand-alone binary, nothing preloaded.  Then the binding:
the setter is exported, declared, bound, and refuses other values than 0 / 1."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT
from versalignlib_amd import build as b
from versalignlib_amd import hipkernel

SRC = os.path.join(ROOT, "tests", "extend_wide_rules_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "valign_hip.h")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + ["-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "extend wide rules ok" in res.stdout, res.stdout[-3000:]
    assert "runtime error" not in res.stdout and "AddressSanitizer" not in res.stdout, res.stdout[-3000:]


def test_extend_wide_rules_check(tmp_path):
    _build_and_run(tmp_path, "extend_wide_rules_check", [])


def test_extend_wide_rules_check_under_asan_and_ubsan(tmp_path):
    _build_and_run(tmp_path, "extend_wide_rules_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_the_rule_lives_in_the_header_alone():
    rules = open(os.path.join(CSRC, "cell_rules.h")).read()
    assert len(re.findall(r"\binline\s+bool\s+extend_int32_ok\s*\(", rules)) == 1
    fields = [line for line in rules[rules.index("struct PlacedFacts"):rules.index("struct PlacedChoice")].splitlines() if " = " in line]
    assert "bool extend_wide = false;" in fields[-1]              # trailing: the aggregate initialisers from before the key stay valid
    for unit in ("engine.hip.h", "engine_core.hip", "engine_placed.hip", "engine_extend.hip", "hip_plugin.hip", "extend_wide_kernels.hip.h"):
        text = open(os.path.join(CSRC, unit)).read()
        assert not re.search(r"\binline\s+\w[\w ]*\s+extend_int32_ok\s*\(", text), unit
        assert "extend_wide: shape" not in text, unit              # (the refusal's text lives in the header)
    # one strip loop for placed and extension scores
    units = [open(os.path.join(CSRC, u)).read() for u in ("engine_placed.hip", "engine_extend.hip")]
    assert units[0].count("void Engine::score_placed_strips(") == 1 and "score_placed_strips(extend_wide_sweep(" in units[1]
    assert "plan.strips" not in units[1]


def test_setter_is_exported_declared_and_bound():
    if not os.path.exists(b.HIP_PLUGIN):
        b.build_hip()
    sym = "valign_hip_set_extend_wide"
    assert hasattr(ctypes.CDLL(b.HIP_PLUGIN), sym) and sym in hipkernel.EXPORTED_SYMBOLS
    L = hipkernel.lib()
    assert L.valign_hip_set_extend_wide.argtypes == [ctypes.c_void_p, ctypes.c_int]
    # a null engine is refused with a message, without a device
    assert L.valign_hip_set_extend_wide(None, 1) != 0 and b"null engine" in L.valign_hip_last_error()
    assert callable(hipkernel.Engine.set_extend_wide)
    text = open(HEADER).read()
    assert re.search(r"\bint\s+valign_hip_set_extend_wide\s*\(\s*valign_hip_engine\s*\*\s*e\s*,\s*int\s+on\s*\)\s*;", text)
    flat = " ".join(" ".join(re.sub(r"^\s*/?\*+\s?", "", line) for line in text.splitlines()).split())
    for phrase in ("key extend_wide", "\"extend_wide:\"", "Other values than 0 / 1 are refused", "\"wide\" (extend_wide"):
        assert phrase in flat, phrase
    # other values than 0 / 1: refused by the engine's setter, as the other keys' are
    engine = open(os.path.join(CSRC, "engine.hip.h")).read()
    assert re.search(r"void set_extend_wide\(int on\) \{\s*if \(on != 0 && on != 1\) throw std::runtime_error\(\"extend_wide must be 0 or 1\"\);", engine)
    plugin = open(os.path.join(CSRC, "hip_plugin.hip")).read()
    assert "e->impl->set_extend_wide(on)" in plugin
    assert "extend_wide_kernels.hip.h" in b.HIP_HEADERS
