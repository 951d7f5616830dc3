"""The suboptimal-score entry points exist: libHIPKernel.so exports both symbols, include/valign_hip.h declares them with the
stated definition, hipkernel binds them, and valign_hip_subopt is 20 bytes for a C caller (a tiny g++ program over the public
header).  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from versalignlib_amd import build as b
from versalignlib_amd import hipkernel

HEADER = os.path.join(ROOT, "include", "valign_hip.h")
SYMBOLS = ("valign_hip_score_subopt_device", "valign_hip_score_subopt_host")


def test_library_exports_the_subopt_entry_points():
    if not os.path.exists(b.HIP_PLUGIN):
        b.build_hip()
    lib = ctypes.CDLL(b.HIP_PLUGIN)
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in hipkernel.EXPORTED_SYMBOLS, sym
    L = hipkernel.lib()
    vp = ctypes.c_void_p
    assert L.valign_hip_score_subopt_device.argtypes == [vp, ctypes.c_int, ctypes.c_longlong, vp, vp, ctypes.c_int, vp, vp]
    assert L.valign_hip_score_subopt_host.argtypes == [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_int]
    # a null engine is refused with a message, without a device
    assert L.valign_hip_score_subopt_device(None, 0, 1, None, None, 0, None, None) != 0
    assert b"null engine" in L.valign_hip_last_error()
    assert L.valign_hip_score_subopt_host(None, 0, 1, None, None, 0, None, 1) != 0
    assert b"null engine" in L.valign_hip_last_error()
    assert callable(hipkernel.Engine.score_subopt_device) and callable(hipkernel.Engine.score_subopt_host)


def test_header_declares_them_and_states_the_definition():
    text = open(HEADER).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(\s*valign_hip_engine\s*\*", text), sym
    assert re.search(r"typedef\s+struct\s*\{[^}]*int32_t\s+score\s*,\s*read_end\s*,\s*ref_end\s*,\s*score2\s*,\s*ref_end2\s*;[^}]*\}\s*valign_hip_subopt\s*;", text)
    flat = " ".join(" ".join(re.sub(r"^\s*/?\*+\s?", "", line) for line in text.splitlines()).split())      # comment text, line frames removed
    for phrase in ("exactly what valign_hip_score_placed_device returns", "last ACGT byte (either case)", "0 <= j < Fp", "0 <= i < Rp",
                   "|j - (ref_end - 1)| > mask", "SMALLEST candidate column", "no candidate or the largest is 0", "five zeros",
                   "THE CALLER PICKS THE MASK", "half the read length", "mask < 0", "WHATEVER band_placed says",
                   "placed_wide = 1 does not open", "more than 1024 rows", "ran_subopt", "subopt_scratch_bytes", "subopt_ring_cols",
                   "belong on one stream"):
        assert phrase in flat, phrase
    # the struct's name never stands in front of a parenthesis (tests/test_host_and_abi.py collects such names as functions)
    assert not re.search(r"valign_hip_subopt\s*\(", text)


def test_record_is_twenty_bytes_for_a_c_caller(tmp_path):
    src = tmp_path / "subopt_size.cpp"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include <type_traits>\n#include "valign_hip.h"\n'
                   "static_assert(sizeof(valign_hip_subopt) == 20, \"20 bytes\");\n"
                   "static_assert(std::is_same<decltype(&valign_hip_score_subopt_device), int (*)(valign_hip_engine *, int, long long, "
                   "const void *, const void *, int, void *, void *)>::value, \"device signature\");\n"
                   "static_assert(std::is_same<decltype(&valign_hip_score_subopt_host), int (*)(valign_hip_engine *, int, int, "
                   "const char *const *, const char *const *, int, valign_hip_subopt *, int)>::value, \"host signature\");\n"
                   'int main() { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(valign_hip_subopt), offsetof(valign_hip_subopt, score), '
                   "offsetof(valign_hip_subopt, read_end), offsetof(valign_hip_subopt, ref_end), offsetof(valign_hip_subopt, score2), "
                   "offsetof(valign_hip_subopt, ref_end2)); return 0; }\n")
    exe = str(tmp_path / "subopt_size")
    build = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == ["20", "0", "4", "8", "12", "16"], res.stdout
    dt = hipkernel.subopt_dtype()
    assert dt.itemsize == 20 and dt.names == ("score", "read_end", "ref_end", "score2", "ref_end2")
    assert np.dtype(dt).fields["ref_end2"][1] == 16


def test_build_lists_and_instances():
    assert "engine_subopt.hip" in b.HIP_SOURCES and "subopt_kernels.hip.h" in b.HIP_HEADERS
    assert "subopt_kernels.hip.h" not in b.KERNEL_PART_DEPS          # (the per-geometry kernel parts do not see it)
    csrc = os.path.join(ROOT, "versalignlib_amd", "csrc")
    inst = open(os.path.join(csrc, "kernel_instances.hip.h")).read()
    assert inst.index("#define VALIGN_SUBOPT_KERNELS") > inst.index("#define VALIGN_PLACED_KERNELS")
    part = open(os.path.join(csrc, "kernel_part.hip")).read()
    assert part.count("VALIGN_SUBOPT_KERNELS(template, G, K, true)") == 1 and part.count("VALIGN_SUBOPT_KERNELS(template, G, K, false)") == 1
