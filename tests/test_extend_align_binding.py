"""The extension-alignment entry points exist: libHIPKernel.so exports both symbols, include/valign_hip.h declares them with the
stated definition and signatures (a tiny g++ program over the public header), hipkernel binds them, a null engine is refused, the
build lists name the new unit and header, and the lookup holds its 12 instances.  No GPU."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT
from versalignlib_amd import build as b
from versalignlib_amd import hipkernel

HEADER = os.path.join(ROOT, "include", "valign_hip.h")
SYMBOLS = ("valign_hip_align_extend_device", "valign_hip_align_extend_host")


def test_library_exports_the_extend_align_entry_points():
    if not os.path.exists(b.HIP_PLUGIN):
        b.build_hip()
    lib = ctypes.CDLL(b.HIP_PLUGIN)
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in hipkernel.EXPORTED_SYMBOLS, sym
    L = hipkernel.lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert L.valign_hip_align_extend_device.argtypes == [vp, ci, ctypes.c_longlong, vp, vp, ci, ci, vp, vp, ci, vp, vp]
    assert L.valign_hip_align_extend_host.argtypes == [vp, ci, ci, vp, vp, ci, ci, vp, vp, ctypes.c_longlong, vp, vp, vp, ci]
    # a null engine is refused with a message, without a device
    assert L.valign_hip_align_extend_device(None, 0, 1, None, None, -1, 0, None, None, 1, None, None) != 0
    assert b"null engine" in L.valign_hip_last_error()
    assert L.valign_hip_align_extend_host(None, 0, 1, None, None, -1, 0, None, None, 0, None, None, None, 1) != 0
    assert b"null engine" in L.valign_hip_last_error()
    assert callable(hipkernel.Engine.align_extend_device) and callable(hipkernel.Engine.align_extend_host)


def test_header_declares_them_and_states_the_definition():
    text = open(HEADER).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(\s*valign_hip_engine\s*\*", text), sym
    flat = " ".join(" ".join(re.sub(r"^\s*/?\*+\s?", "", line) for line in text.splitlines()).split())      # comment text, line frames removed
    for phrase in ("end_bonus < 0: the best cell (read_end - 1, ref_end - 1)", "(int64) gscore + end_bonus >= score", "the border column -1",
                   "end_bonus = INT32_MAX means \"always the read end\"", "Ties go to the read end", "an all-zero record and no ops",
                   "back to (-1, -1)", "X(i,j) == X(i-1,j-1) + S(i,j)", "X(i,j) == X(i-1,j) + gap_ref", "else LEFT", "three-state rule",
                   "f != f_open, e != e_open", "UP on column -1, LEFT on row -1", "a gap run that turns the corner opens again",
                   "A first op of I or D is legal", "read_begin = ref_begin = 0", "ref_end = 0 for the border column", "score == X(end cell)",
                   "consume exactly read_end read bases and ref_end reference bases", "without a literal '-' byte",
                   "bit for bit what valign_hip_score_extend_device returns", "begins \"extension alignments:\"", "extended not 0 or 1",
                   "ops_stride < 1", "null result buffers", "ran_extend_align", "ran_extend_align_geometry", "extend_align_scratch_bytes",
                   "Z-drop / X-drop", "pointer_scratch_cap_mb", "tests/extend_align_ref.py"):
        assert phrase in flat, phrase


def test_signatures_for_a_c_caller(tmp_path):
    src = tmp_path / "extend_align_sig.cpp"
    src.write_text('#include <stdint.h>\n#include <type_traits>\n#include "valign_hip.h"\n'
                   "static_assert(std::is_same<decltype(&valign_hip_align_extend_device), int (*)(valign_hip_engine *, int, long long, "
                   "const void *, const void *, int, int, void *, void *, int, void *, void *)>::value, \"device signature\");\n"
                   "static_assert(std::is_same<decltype(&valign_hip_align_extend_host), int (*)(valign_hip_engine *, int, int, "
                   "const char *const *, const char *const *, int, int, valign_hip_aln *, uint32_t *, long long, long long *, long long *, "
                   "valign_hip_extend *, int)>::value, \"host signature\");\n"
                   "int main() { return 0; }\n")
    exe = str(tmp_path / "extend_align_sig")
    build = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    assert subprocess.run([exe], timeout=120).returncode == 0


def test_build_lists_and_instances():
    assert "engine_extend_align.hip" in b.HIP_SOURCES and "extend_align_kernels.hip.h" in b.HIP_HEADERS
    assert "extend_align_kernels.hip.h" in b.KERNEL_PART_DEPS              # (the per-geometry kernel parts compile it)
    csrc = os.path.join(ROOT, "versalignlib_amd", "csrc")
    inst = open(os.path.join(csrc, "kernel_instances.hip.h")).read()
    assert inst.index("#define VALIGN_EXTEND_ALIGN_KERNELS") > inst.index("#define VALIGN_EXTEND_KERNELS")
    assert '#include "extend_align_kernels.hip.h"' in inst
    part = open(os.path.join(csrc, "kernel_part.hip")).read()
    assert part.count("VALIGN_EXTEND_ALIGN_KERNELS(template, G, K, true)") == 1 and part.count("VALIGN_EXTEND_ALIGN_KERNELS(template, G, K, false)") == 1
    kernels = open(os.path.join(csrc, "extend_align_kernels.hip.h")).read()
    # two forms on each full geometry: 2 x 6 = 12 instances, assigned under `if constexpr (FULL)`
    assigned = re.findall(r"fill\[(\d)\]\s*=\s*\(const void \*\)&align_extend_fill_kernel<G, K, (false|true)>;", kernels)
    assert sorted(assigned) == [("0", "false"), ("1", "true")], assigned
    assert re.search(r"if constexpr \(FULL\) \{\s*fill\[0\]", kernels)
    full = re.findall(r"full_geometry<(\d+), (\d+)>\(\)", open(os.path.join(csrc, "engine.hip.h")).read())
    assert len(set(full)) == 6 and len(assigned) * len(set(full)) == 12
    engine = open(os.path.join(csrc, "engine.hip.h")).read()
    assert "&extend_align_kernel<G, K, true>" in engine and "&extend_align_kernel<G, K, false>" in engine
    # the existing walk and sweeps know nothing of this path: it reuses their helpers from its own header
    for name in ("trace_kernels.hip.h", "extend_kernels.hip.h", "cigar_kernels.hip.h"):
        text = open(os.path.join(csrc, name)).read()
        assert "extend_align" not in text and "ExtendAlign" not in text and "ExtendWalk" not in text, name
