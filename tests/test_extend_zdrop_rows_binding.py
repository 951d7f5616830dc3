"""The extend_zdrop_rows key exists: libHIPKernel.so exports valign_hip_set_extend_zdrop_rows, include/valign_hip.h declares it in a
section below the extend_zdrop one and qualifies that section's two sentences about the register sweep there, hipkernel binds it, a
null engine is refused with a message, describe() carries the key, and the 24 + 12 ZDROP instances of the register sweep sit in
lookup functions of their own beside the plain ones.  No GPU."""
import ctypes
import os
import re

from conftest import ROOT
from versalignlib_amd import build as b
from versalignlib_amd import hipkernel

HEADER = os.path.join(ROOT, "include", "valign_hip.h")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")
SYM = "valign_hip_set_extend_zdrop_rows"


def test_setter_is_exported_and_bound():
    if not os.path.exists(b.HIP_PLUGIN):
        b.build_hip()
    assert hasattr(ctypes.CDLL(b.HIP_PLUGIN), SYM) and SYM in hipkernel.EXPORTED_SYMBOLS
    L = hipkernel.lib()
    assert L.valign_hip_set_extend_zdrop_rows.argtypes == [ctypes.c_void_p, ctypes.c_int]
    # a null engine is refused with a message, without a device
    for on in (0, 1, 2, -1):
        assert L.valign_hip_set_extend_zdrop_rows(None, on) != 0 and b"null engine" in L.valign_hip_last_error()
    assert callable(hipkernel.Engine.set_extend_zdrop_rows)
    # 0 or 1: the engine's setter refuses everything else with the rule header's text
    engine = open(os.path.join(CSRC, "engine.hip.h")).read()
    assert re.search(r"void set_extend_zdrop_rows\(int on\) \{\s*if \(!extend_zdrop_rows_key_ok\(on\)\) throw std::runtime_error\(kExtendZdropRowsKeyRange\);", engine)
    assert 'kExtendZdropRowsKeyRange = "extend_zdrop_rows must be 0 or 1"' in open(os.path.join(CSRC, "extend_zdrop.h")).read()
    assert "e->impl->set_extend_zdrop_rows(on)" in open(os.path.join(CSRC, "hip_plugin.hip")).read()
    assert '\\"extend_zdrop_rows\\": ' in open(os.path.join(CSRC, "engine_core.hip")).read()
    # the kernel parts are rebuilt when the rule header changes
    assert "extend_zdrop.h" in b.KERNEL_PART_DEPS and "extend_zdrop.h" in b.HIP_HEADERS


def test_the_zdrop_instances_have_lookups_of_their_own():
    scores = open(os.path.join(CSRC, "extend_kernels.hip.h")).read()
    fills = open(os.path.join(CSRC, "extend_align_kernels.hip.h")).read()
    forms = re.findall(r"^\s*dropping\[(\w+)\] = \(const void \*\)&score_extend_kernel<G, K, (\w+), true>;", scores, flags=re.M)
    assert sorted(forms) == sorted((f, f) for f in ("kGapLinear", "kGapSym", "kGapAffine", "kGapAffineSym"))         # x six full geometries: 24
    assert re.findall(r"^\s*dropping\[(\d)\] = \(const void \*\)&align_extend_fill_kernel<G, K, (\w+), true>;", fills, flags=re.M) == [("0", "false"), ("1", "true")]      # 12
    table = open(os.path.join(CSRC, "engine.hip.h")).read()
    for full in ("true", "false"):
        assert "&extend_zdrop_kernel<G, K, %s>, &extend_align_zdrop_kernel<G, K, %s>" % (full, full) in table
    part = open(os.path.join(CSRC, "kernel_part.hip")).read()
    assert part.count("VALIGN_EXTEND_ZDROP_KERNELS(template, G, K, true)") == 1 and part.count("VALIGN_EXTEND_ZDROP_KERNELS(template, G, K, false)") == 1
    # the engine launches them on the plan of the plain instances
    assert "plan.geo->extend_zdrop(gaps)" in open(os.path.join(CSRC, "engine_extend.hip")).read()
    assert "plan.geo->extend_align_zdrop(" in open(os.path.join(CSRC, "engine_extend_align.hip")).read()


def test_header_section_sits_below_the_extend_zdrop_one():
    text = open(HEADER).read()
    decl = re.search(r"\bint\s+valign_hip_set_extend_zdrop_rows\s*\(\s*valign_hip_engine\s*\*\s*e\s*,\s*int\s+on\s*\)\s*;", text)
    assert decl and decl.start() > text.index("int valign_hip_set_extend_zdrop(") and decl.start() < text.index("int valign_hip_host_register(")
    flat = " ".join(" ".join(re.sub(r"^\s*/?\*+\s?", "", line) for line in text.splitlines()).split())      # comment text, line frames removed
    section = flat[flat.index("Extension Z-drop on the int16 register sweep"):flat.index("int valign_hip_set_extend_zdrop_rows(")]
    for phrase in ("key extend_zdrop_rows; flat API only", "\"extend_zdrop_rows must be 0 or 1\"", "only where extend_zdrop > 0 and band_width == 0",
                   "Z = 0 under the key is the call without either key", "\"ran_extend\": \"rows\"", "score_width = 16 included", "\"ran_extend_align\": \"rows\"",
                   "the int32 route of unbanded extension alignments has no Z-drop form", "The banded route answers as above", "exclusive prefix arg-max",
                   "T is the smallest row any lane answers", "No cell, no back pointer and no step of the sweep changes", "no in-sweep stop",
                   "the read end is picked only where nothing dropped", "0 <= M - m_i <= 65535", "M - m_i - pen lies in (-2^30, 2^16)",
                   "\"extend_zdrop_skipped_waves\" is 0", "tests/extend_zdrop_ref.py", "tests/extend_align_ref.py"):
        assert phrase in section, phrase
    # the two older sentences stand as they were, above, qualified by the section
    for phrase in ("KNOWN: the int16 register sweep has no Z-drop form, so a 150-row read under the key fills 150 of its strip's 512 rows",
                   "NOT BUILT: a Z-drop form of the int16 register sweep; an in-strip stop; an anti-diagonal (ksw_extz-style) rule"):
        assert phrase in flat and flat.index(phrase) < flat.index("Extension Z-drop on the int16 register sweep"), phrase
    assert "\"KNOWN: the int16 register sweep has no Z-drop form\" and \"NOT BUILT: a Z-drop form of the int16 register sweep\" are qualified here" in section
