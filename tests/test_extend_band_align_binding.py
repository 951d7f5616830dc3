"""The extend_band_align key exists: libHIPKernel.so exports valign_hip_set_extend_band_align, include/valign_hip.h declares it in a
section below the extension alignments' and states the definition there, hipkernel binds it, a null engine is refused with a
message, and the sentences of the older sections stand as they were.  No GPU."""
import ctypes
import os
import re

from conftest import ROOT
from versalignlib_amd import build as b
from versalignlib_amd import hipkernel

HEADER = os.path.join(ROOT, "include", "valign_hip.h")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")
SYM = "valign_hip_set_extend_band_align"


def test_setter_is_exported_and_bound():
    if not os.path.exists(b.HIP_PLUGIN):
        b.build_hip()
    assert hasattr(ctypes.CDLL(b.HIP_PLUGIN), SYM) and SYM in hipkernel.EXPORTED_SYMBOLS
    L = hipkernel.lib()
    assert L.valign_hip_set_extend_band_align.argtypes == [ctypes.c_void_p, ctypes.c_int]
    # a null engine is refused with a message, without a device
    assert L.valign_hip_set_extend_band_align(None, 1) != 0 and b"null engine" in L.valign_hip_last_error()
    assert callable(hipkernel.Engine.set_extend_band_align)
    engine = open(os.path.join(CSRC, "engine.hip.h")).read()
    assert re.search(r"void set_extend_band_align\(int on\) \{\s*if \(on != 0 && on != 1\) throw std::runtime_error\(\"extend_band_align must be 0 or 1\"\);", engine)
    assert "e->impl->set_extend_band_align(on)" in open(os.path.join(CSRC, "hip_plugin.hip")).read()
    core = open(os.path.join(CSRC, "engine_core.hip")).read()
    assert '\\"extend_band_align\\": ' in core and '\\"ran_extend_align_chunks\\": ' in core
    assert "extend_band_align_plan.h" in b.HIP_HEADERS and "extend_band_align_kernels.hip.h" in b.HIP_HEADERS
    assert "extend_band_align_plan.h" in b.KERNEL_PART_DEPS and "extend_band_plan.h" in b.KERNEL_PART_DEPS      # (cell_rules.h includes them)
    # the two fill instances live in the extension-alignment unit, the sweep's body in the score sweep's header
    unit = open(os.path.join(CSRC, "engine_extend_align.hip")).read()
    assert "align_extend_band_fill_kernel<K, true>" in unit and "align_extend_band_fill_kernel<K, false>" in unit
    assert "extend_band_ends_kernel" in unit and "extend_band_walk_kernel" in unit and "cigar_encode_kernel" in unit
    sweep = open(os.path.join(CSRC, "extend_wide_kernels.hip.h")).read()
    assert "template <int K, bool AFFINE, bool BANDED = false, bool PTRS = false>" in sweep and sweep.count("if constexpr (PTRS)") >= 4
    assert "&score_extend_wide_kernel<K, AFFINE, true, true>" in open(os.path.join(CSRC, "extend_band_align_kernels.hip.h")).read()


def test_header_states_the_definition_below_the_extension_alignments():
    text = open(HEADER).read()
    decl = re.search(r"\bint\s+valign_hip_set_extend_band_align\s*\(\s*valign_hip_engine\s*\*\s*e\s*,\s*int\s+on\s*\)\s*;", text)
    assert decl and decl.start() > text.index("int valign_hip_align_extend_host(") and decl.start() < text.index("int valign_hip_host_register(")
    flat = " ".join(" ".join(re.sub(r"^\s*/?\*+\s?", "", line) for line in text.splitlines()).split())      # comment text, line frames removed
    for phrase in ("key extend_band_align; flat API only", "1 with band_width > 0 and extend_band = 1", "whatever the read length, score_width (0 or 32) or extend_wide say",
                   "With band_width == 0 or extend_band == 0 the key is not read", "No other call reads the key", "\"extend_band_align must be 0 or 1\"",
                   "exactly those of banded extension scores", "bit for bit what valign_hip_score_extend_device returns under the same keys",
                   "gscore = VALIGN_HIP_EXTEND_UNREACHED, gref_end = 0 for an unreached read end", "computed in 64 bits",
                   "An unreached read end is never chosen, whatever end_bonus is", "INT32_MIN + INT32_MAX = -1 < 0 <= score",
                   "\"the read end wherever it is reached\"", "|gscore| < 2^28 on this route", "the best cell was chosen and score == 0, or Rp == 0",
                   "an absent candidate equals nothing", "(i, -1) present implies (i-1, -1) present", "(-1, j) present implies (-1, j-1) present",
                   "every present interior cell has a present candidate", "the walk never leaves the band", "score == X_band(end cell)",
                   "consume exactly read_end read bases and ref_end reference bases", "literal-'-' caveat", "w >= max(R, F) gives the unbanded extension alignment",
                   "tests/extend_align_ref.py restates it", "ops_cap / ops_needed", "opt & 0xF == 1 and traceback_policy = 1, with their texts",
                   "score_width = 16, with the text that begins \"extend_band:\"", "extended not 0 or 1; ops_stride < 1; null result buffers",
                   "NOT BUILT, still: Z-drop / X-drop", "a register (int16, sub-wave) form of the band", "\"ran_extend_align\": \"band\"",
                   "\"ran_extend_align_geometry\": \"none\"", "\"align_ptr_bytes_per_pair\" the band's pointer bytes per pair", "\"extend_align_scratch_bytes\"",
                   "pointer_scratch_cap_mb", "tests/extend_band_align_ref.py"):
        assert phrase in flat, phrase
    # the older sentences stand as they were
    for phrase in ("Z-drop, and extension alignments under a band or on int32 cells, remain unbuilt", "NOT BUILT: Z-drop / X-drop, a band around the anchor's diagonal, the int32 route",
                   "|gscore| <= 32000 on this route, so end_bonus = INT32_MAX means \"always the read end\"", "extension alignments (below) refuse the calls this key moves to the int32 sweep",
                   "text that starts \"extension alignments: not built under a band\"", "\"ran_extend_align\" of valign_hip_describe is \"rows\" after a call that ran"):
        assert phrase in flat, phrase
