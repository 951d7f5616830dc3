"""The extension-score entry points exist: libHIPKernel.so exports both symbols, include/valign_hip.h declares them with the
stated definition, hipkernel binds them, and valign_hip_extend is 20 bytes for a C caller (a tiny g++ program over the public
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
SYMBOLS = ("valign_hip_score_extend_device", "valign_hip_score_extend_host")


def test_library_exports_the_extend_entry_points():
    if not os.path.exists(b.HIP_PLUGIN):
        b.build_hip()
    lib = ctypes.CDLL(b.HIP_PLUGIN)
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in hipkernel.EXPORTED_SYMBOLS, sym
    L = hipkernel.lib()
    vp = ctypes.c_void_p
    assert L.valign_hip_score_extend_device.argtypes == [vp, ctypes.c_int, ctypes.c_longlong, vp, vp, vp, vp]
    assert L.valign_hip_score_extend_host.argtypes == [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int]
    # a null engine is refused with a message, without a device
    assert L.valign_hip_score_extend_device(None, 0, 1, None, None, None, None) != 0
    assert b"null engine" in L.valign_hip_last_error()
    assert L.valign_hip_score_extend_host(None, 0, 1, None, None, None, 1) != 0
    assert b"null engine" in L.valign_hip_last_error()
    assert callable(hipkernel.Engine.score_extend_device) and callable(hipkernel.Engine.score_extend_host)


def test_header_declares_them_and_states_the_definition():
    text = open(HEADER).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(\s*valign_hip_engine\s*\*", text), sym
    assert re.search(r"typedef\s+struct\s*\{[^}]*int32_t\s+score\s*,\s*read_end\s*,\s*ref_end\s*,\s*gscore\s*,\s*gref_end\s*;[^}]*\}\s*valign_hip_extend\s*;", text)
    flat = " ".join(" ".join(re.sub(r"^\s*/?\*+\s?", "", line) for line in text.splitlines()).split())      # comment text, line frames removed
    for phrase in ("starts before read[0] and ref[0]", "THE CALLER PASSES THE SEQUENCE AFTER ITS SEED", "the caller reverses both sequences",
                   "last ACGT byte (either case)", "X(-1,-1) = 0", "(i + 1) * gap_ref", "open_ref + i * ext_ref", "(j + 1) * gap_read",
                   "open_read + j * ext_read", "NO FLOOR AT ZERO", "open + (k - 1) * ext", "0 <= i < Rp, 0 <= j < Fp", "row-major first cell",
                   "score = read_end = ref_end = 0", "-1 <= j < Fp", "the border column counts as j = -1", "may be negative",
                   "smallest candidate column", "five zeros", "Columns at or beyond Fp are not candidates", "Z-drop or X-drop termination",
                   "every cell is swept", "gscore + bonus", "ragged_batching and half_float_cells are not read", "opt & 0xF == 1",
                   "traceback_policy = 1", "WHATEVER band_placed says", "WHATEVER placed_wide says", "could leave int16", "more than 1024 rows",
                   "opt & 0xF > 1 does nothing", "ran_extend"):
        assert phrase in flat, phrase
    # the struct's name never stands in front of a parenthesis (tests/test_host_and_abi.py collects such names as functions)
    assert not re.search(r"valign_hip_extend\s*\(", text)


def test_record_is_twenty_bytes_for_a_c_caller(tmp_path):
    src = tmp_path / "extend_size.cpp"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include <type_traits>\n#include "valign_hip.h"\n'
                   "static_assert(sizeof(valign_hip_extend) == 20, \"20 bytes\");\n"
                   "static_assert(std::is_same<decltype(&valign_hip_score_extend_device), int (*)(valign_hip_engine *, int, long long, "
                   "const void *, const void *, void *, void *)>::value, \"device signature\");\n"
                   "static_assert(std::is_same<decltype(&valign_hip_score_extend_host), int (*)(valign_hip_engine *, int, int, "
                   "const char *const *, const char *const *, valign_hip_extend *, int)>::value, \"host signature\");\n"
                   'int main() { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(valign_hip_extend), offsetof(valign_hip_extend, score), '
                   "offsetof(valign_hip_extend, read_end), offsetof(valign_hip_extend, ref_end), offsetof(valign_hip_extend, gscore), "
                   "offsetof(valign_hip_extend, gref_end)); return 0; }\n")
    exe = str(tmp_path / "extend_size")
    build = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == ["20", "0", "4", "8", "12", "16"], res.stdout
    dt = hipkernel.extend_dtype()
    assert dt.itemsize == 20 and dt.names == ("score", "read_end", "ref_end", "gscore", "gref_end")
    assert np.dtype(dt).fields["gref_end"][1] == 16


def test_build_lists_and_instances():
    assert "engine_extend.hip" in b.HIP_SOURCES and "extend_kernels.hip.h" in b.HIP_HEADERS
    assert "extend_kernels.hip.h" in b.KERNEL_PART_DEPS              # (the per-geometry kernel parts compile it)
    csrc = os.path.join(ROOT, "versalignlib_amd", "csrc")
    inst = open(os.path.join(csrc, "kernel_instances.hip.h")).read()
    assert inst.index("#define VALIGN_EXTEND_KERNELS") > inst.index("#define VALIGN_SUBOPT_KERNELS")
    assert '#include "extend_kernels.hip.h"' in inst
    part = open(os.path.join(csrc, "kernel_part.hip")).read()
    assert part.count("VALIGN_EXTEND_KERNELS(template, G, K, true)") == 1 and part.count("VALIGN_EXTEND_KERNELS(template, G, K, false)") == 1
    kernels = open(os.path.join(csrc, "extend_kernels.hip.h")).read()
    for form in ("kGapLinear", "kGapSym", "kGapAffine", "kGapAffineSym"):
        assert "score_extend_kernel<G, K, %s>" % form in kernels, form
