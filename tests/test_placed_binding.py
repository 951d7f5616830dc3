"""The placed-score entry points exist: libHIPKernel.so exports both symbols, include/valign_hip.h declares them with the
stated definition, and valign_hip_placed is 12 bytes for a C caller (a tiny g++ program over the public header).  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from versalignlib_amd import build as b
from versalignlib_amd import hipkernel

HEADER = os.path.join(ROOT, "include", "valign_hip.h")
SYMBOLS = ("valign_hip_score_placed_device", "valign_hip_score_placed_host")


def test_library_exports_the_placed_entry_points():
    if not os.path.exists(b.HIP_PLUGIN):
        b.build_hip()
    lib = ctypes.CDLL(b.HIP_PLUGIN)
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in hipkernel.EXPORTED_SYMBOLS, sym
    # a null engine is refused with a message, without a device
    L = hipkernel.lib()
    assert L.valign_hip_score_placed_device(None, 0, 1, None, None, None, None) != 0
    assert b"null engine" in L.valign_hip_last_error()
    assert L.valign_hip_score_placed_host(None, 0, 1, None, None, None, 1) != 0


def test_header_declares_them_and_states_the_definition():
    text = open(HEADER).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(\s*valign_hip_engine\s*\*", text), sym
    assert re.search(r"typedef\s+struct\s*\{[^}]*int32_t\s+score\s*,\s*read_end\s*,\s*ref_end\s*;[^}]*\}\s*valign_hip_placed\s*;", text)
    for phrase in ("DefaultKernel.cpp:252-256", "half-open", "{0, 0, 0}", "band_width > 0", "traceback_policy = 1", "score_width = 32",
                   "opt & 0xF == 1", "ran_placed"):
        assert phrase in text, phrase


def test_record_is_twelve_bytes_for_a_c_caller(tmp_path):
    src = tmp_path / "placed_size.cpp"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include <type_traits>\n#include "valign_hip.h"\n'
                   "static_assert(sizeof(valign_hip_placed) == 12, \"12 bytes\");\n"
                   "static_assert(std::is_same<decltype(&valign_hip_score_placed_device), int (*)(valign_hip_engine *, int, long long, "
                   "const void *, const void *, void *, void *)>::value, \"device signature\");\n"
                   "static_assert(std::is_same<decltype(&valign_hip_score_placed_host), int (*)(valign_hip_engine *, int, int, "
                   "const char *const *, const char *const *, valign_hip_placed *, int)>::value, \"host signature\");\n"
                   'int main() { printf("%zu %zu %zu %zu\\n", sizeof(valign_hip_placed), offsetof(valign_hip_placed, score), '
                   "offsetof(valign_hip_placed, read_end), offsetof(valign_hip_placed, ref_end)); return 0; }\n")
    exe = str(tmp_path / "placed_size")
    build = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == ["12", "0", "4", "8"], res.stdout
    assert hipkernel.placed_dtype().itemsize == 12 and hipkernel.placed_dtype().names == ("score", "read_end", "ref_end")
    assert np.dtype(hipkernel.placed_dtype()).fields["ref_end"][1] == 8
