"""The extend_band key exists: libHIPKernel.so exports valign_hip_set_extend_band, include/valign_hip.h declares it below the
extend_wide section and states the band's definition, hipkernel binds it, a null engine is refused with a message, and the two
#defines are visible to a C caller (a tiny g++ program over the public header).  No GPU."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT
from versalignlib_amd import build as b
from versalignlib_amd import hipkernel

HEADER = os.path.join(ROOT, "include", "valign_hip.h")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")
SYM = "valign_hip_set_extend_band"


def test_setter_is_exported_and_bound():
    if not os.path.exists(b.HIP_PLUGIN):
        b.build_hip()
    assert hasattr(ctypes.CDLL(b.HIP_PLUGIN), SYM) and SYM in hipkernel.EXPORTED_SYMBOLS
    L = hipkernel.lib()
    assert L.valign_hip_set_extend_band.argtypes == [ctypes.c_void_p, ctypes.c_int]
    # a null engine is refused with a message, without a device
    assert L.valign_hip_set_extend_band(None, 1) != 0 and b"null engine" in L.valign_hip_last_error()
    assert callable(hipkernel.Engine.set_extend_band)
    assert hipkernel.EXTEND_BAND_BLOCK_ROWS == 8 and hipkernel.EXTEND_UNREACHED == -2 ** 31
    # other values than 0 / 1: refused by the engine's setter, as the other keys' are
    engine = open(os.path.join(CSRC, "engine.hip.h")).read()
    assert re.search(r"void set_extend_band\(int on\) \{\s*if \(on != 0 && on != 1\) throw std::runtime_error\(\"extend_band must be 0 or 1\"\);", engine)
    assert "e->impl->set_extend_band(on)" in open(os.path.join(CSRC, "hip_plugin.hip")).read()
    core = open(os.path.join(CSRC, "engine_core.hip")).read()
    assert '\\"extend_band\\": %d' in core and '\\"extend_band_block_rows\\": %d' in core
    assert "extend_band_plan.h" in b.HIP_HEADERS


def test_header_states_the_definition_below_the_extend_wide_section():
    text = open(HEADER).read()
    decl = re.search(r"\bint\s+valign_hip_set_extend_band\s*\(\s*valign_hip_engine\s*\*\s*e\s*,\s*int\s+on\s*\)\s*;", text)
    assert decl and decl.start() > text.index("int valign_hip_set_extend_wide(") and decl.start() < text.index("---- extension alignments:")
    flat = " ".join(" ".join(re.sub(r"^\s*/?\*+\s?", "", line) for line in text.splitlines()).split())      # comment text, line frames removed
    for phrase in ("key extend_band; flat API only", "band_width / 2", "band_width = 1 gives w = 0", "B = VALIGN_HIP_EXTEND_BAND_BLOCK_ROWS = 8",
                   "block b holds rows [8b, 8b + 8)", "8*(i/8) - w <= j <= 8*(i/8) + 7 + w", "The border column j = -1 counts like any other column",
                   "cell (-1, j) is present iff j + 1 <= w", "(-1, -1) is always present", "never a candidate of a neighbour, a maximum or an arg-max",
                   "H, E and F are all absent", "hold the unbanded closed-form values", "per-cell band |i - j| <= w", "per-cell band <= result <= unbanded",
                   "w >= max(R, F) gives exactly the unbanded record", "present cells with i < Rp and j < Fp", "present candidates -1 <= j < Fp of row Rp - 1",
                   "8*((Rp-1)/8) - w > Fp - 1", "VALIGN_HIP_EXTEND_UNREACHED (INT32_MIN) and gref_end = 0", "Rp = 0 is still five zeros",
                   "\"ran_extend\": \"band\"", "\"ran_extend_geometry\": \"none\"", "With band_width == 0 the key is not read",
                   "Placed, spanned, suboptimal and alignment calls never read it", "Other values than 0 / 1 are refused", "\"extend_band:\"",
                   "min(R, F) diagonal steps", "extension alignments: not built under a band", "slower than the unbanded int16 register sweep",
                   "\"extend_band_block_rows\"", "tests/extend_band_ref.py"):
        assert phrase in flat, phrase
    # the sentences from before the key stand as they were
    for phrase in ("band_width > 0, WHATEVER band_placed says", "Z-drop and a band around the anchor's diagonal remain unbuilt",
                   "every band_width > 0 stay refused with their texts"):
        assert phrase in flat, phrase


def test_defines_are_visible_to_a_c_caller(tmp_path):
    src = tmp_path / "extend_band_defines.c"
    src.write_text('#include <stdint.h>\n#include <stdio.h>\n#include "valign_hip.h"\n'
                   "#if VALIGN_HIP_EXTEND_BAND_BLOCK_ROWS != 8\n#error block rows\n#endif\n"
                   "#if VALIGN_HIP_EXTEND_UNREACHED != INT32_MIN\n#error unreached\n#endif\n"
                   "int main(void) { int (*set)(valign_hip_engine *, int) = valign_hip_set_extend_band; int32_t u = VALIGN_HIP_EXTEND_UNREACHED; "
                   '(void)set; printf("%d %ld\\n", VALIGN_HIP_EXTEND_BAND_BLOCK_ROWS, (long)u); return 0; }\n')
    exe = str(tmp_path / "extend_band_defines")
    build = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", exe + ".o"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    # (compiled only: the symbol lives in libHIPKernel.so); the values once more through the preprocessor
    pre = subprocess.run(["gcc", "-std=c99", "-E", "-P", "-I" + os.path.join(ROOT, "include"), "-"], input='#include "valign_hip.h"\nROWS VALIGN_HIP_EXTEND_BAND_BLOCK_ROWS UNREACHED VALIGN_HIP_EXTEND_UNREACHED\n',
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert pre.returncode == 0 and "ROWS 8 UNREACHED (-2147483647 - 1)" in pre.stdout, pre.stdout[-500:]
