"""The spanned-score entry points exist: libHIPKernel.so exports both symbols, include/valign_hip.h declares them with the
stated definition, hipkernel binds them, and valign_hip_span is 20 bytes for a C caller (a tiny g++ program over the public
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
SYMBOLS = ("valign_hip_score_span_device", "valign_hip_score_span_host")


def test_library_exports_the_span_entry_points():
    if not os.path.exists(b.HIP_PLUGIN):
        b.build_hip()
    lib = ctypes.CDLL(b.HIP_PLUGIN)
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in hipkernel.EXPORTED_SYMBOLS, sym
    L = hipkernel.lib()
    vp = ctypes.c_void_p
    assert L.valign_hip_score_span_device.argtypes == [vp, ctypes.c_int, ctypes.c_longlong, vp, vp, vp, vp]
    assert L.valign_hip_score_span_host.argtypes == [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int]
    # a null engine is refused with a message, without a device
    assert L.valign_hip_score_span_device(None, 0, 1, None, None, None, None) != 0
    assert b"null engine" in L.valign_hip_last_error()
    assert L.valign_hip_score_span_host(None, 0, 1, None, None, None, 1) != 0
    assert b"null engine" in L.valign_hip_last_error()
    assert callable(hipkernel.Engine.score_span_device) and callable(hipkernel.Engine.score_span_host)


def test_header_declares_them_and_states_the_definition():
    text = open(HEADER).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(\s*valign_hip_engine\s*\*", text), sym
    assert re.search(r"typedef\s+struct\s*\{[^}]*int32_t\s+score\s*,\s*read_begin\s*,\s*read_end\s*,\s*ref_begin\s*,\s*ref_end\s*;[^}]*\}\s*valign_hip_span\s*;", text)
    flat = " ".join(" ".join(re.sub(r"^\s*/?\*+\s?", "", line) for line in text.splitlines()).split())      # comment text, line frames removed
    for phrase in ("prefix rectangle", "only cell of P that holds", "Reverse both prefixes", "FIRST cell in row-major order of the reversed matrix",
                   "read_begin = read_end - 1 - i'", "ref_begin = ref_end - 1 - j'", "latest read row", "five zeros", "GUARANTEED: the global alignment score",
                   "NOT GUARANTEED: equality with valign_hip_aln.read_begin", "not interchangeable", "WHATEVER band_placed says",
                   "span_ref_length", "ran_span", "span_scratch_bytes", "belong on one stream"):
        assert phrase in flat, phrase
    # the struct's name never stands in front of a parenthesis (tests/test_host_and_abi.py collects such names as functions)
    assert not re.search(r"valign_hip_span\s*\(", text)


def test_record_is_twenty_bytes_for_a_c_caller(tmp_path):
    src = tmp_path / "span_size.cpp"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include <type_traits>\n#include "valign_hip.h"\n'
                   "static_assert(sizeof(valign_hip_span) == 20, \"20 bytes\");\n"
                   "static_assert(std::is_same<decltype(&valign_hip_score_span_device), int (*)(valign_hip_engine *, int, long long, "
                   "const void *, const void *, void *, void *)>::value, \"device signature\");\n"
                   "static_assert(std::is_same<decltype(&valign_hip_score_span_host), int (*)(valign_hip_engine *, int, int, "
                   "const char *const *, const char *const *, valign_hip_span *, int)>::value, \"host signature\");\n"
                   'int main() { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(valign_hip_span), offsetof(valign_hip_span, score), '
                   "offsetof(valign_hip_span, read_begin), offsetof(valign_hip_span, read_end), offsetof(valign_hip_span, ref_begin), "
                   "offsetof(valign_hip_span, ref_end)); return 0; }\n")
    exe = str(tmp_path / "span_size")
    build = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == ["20", "0", "4", "8", "12", "16"], res.stdout
    dt = hipkernel.span_dtype()
    assert dt.itemsize == 20 and dt.names == ("score", "read_begin", "read_end", "ref_begin", "ref_end")
    assert np.dtype(dt).fields["ref_end"][1] == 16


def test_build_lists_carry_the_unit_and_the_header():
    assert "engine_span.hip" in b.HIP_SOURCES and "span_kernels.hip.h" in b.HIP_HEADERS
    assert "span_kernels.hip.h" not in b.KERNEL_PART_DEPS          # (the per-geometry kernel parts do not see it)
