"""The extend_zdrop key exists: libHIPKernel.so exports valign_hip_set_extend_zdrop, include/valign_hip.h declares it in a section
below the banded extension alignments' and states the definition there, hipkernel binds it, a null engine is refused with a
message, describe() carries the three fields, and the sentences of the older sections stand as they were.  No GPU."""
import ctypes
import os
import re

from conftest import ROOT
from versalignlib_amd import build as b
from versalignlib_amd import hipkernel

HEADER = os.path.join(ROOT, "include", "valign_hip.h")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")
SYM = "valign_hip_set_extend_zdrop"


def test_setter_is_exported_and_bound():
    if not os.path.exists(b.HIP_PLUGIN):
        b.build_hip()
    assert hasattr(ctypes.CDLL(b.HIP_PLUGIN), SYM) and SYM in hipkernel.EXPORTED_SYMBOLS
    L = hipkernel.lib()
    assert L.valign_hip_set_extend_zdrop.argtypes == [ctypes.c_void_p, ctypes.c_int]
    # a null engine is refused with a message, without a device
    for Z in (0, 10, -1, (1 << 30) + 1):
        assert L.valign_hip_set_extend_zdrop(None, Z) != 0 and b"null engine" in L.valign_hip_last_error()
    assert callable(hipkernel.Engine.set_extend_zdrop)
    # the range is the engine's setter's, its text the rule header's
    engine = open(os.path.join(CSRC, "engine.hip.h")).read()
    assert re.search(r"void set_extend_zdrop\(int Z\) \{\s*if \(!extend_zdrop_key_ok\(Z\)\) throw std::runtime_error\(kExtendZdropKeyRange\);", engine)
    assert 'kExtendZdropKeyRange = "extend_zdrop must be in [0, 2^30]"' in open(os.path.join(CSRC, "extend_zdrop.h")).read()
    assert "e->impl->set_extend_zdrop(Z)" in open(os.path.join(CSRC, "hip_plugin.hip")).read()
    core = open(os.path.join(CSRC, "engine_core.hip")).read()
    for key in ("extend_zdrop", "ran_extend_zdrop", "extend_zdrop_skipped_waves"):
        assert '\\"%s\\": ' % key in core, key
    assert "extend_zdrop.h" in b.HIP_HEADERS
    # the six ZDROP instances: four of the score sweep in the extension unit, two of the fill in the alignment unit
    unit = open(os.path.join(CSRC, "engine_extend.hip")).read()
    for inst in ("<K, true, true, false, true>", "<K, false, true, false, true>", "<K, true, false, false, true>", "<K, false, false, false, true>"):
        assert "score_extend_wide_kernel" + inst in unit, inst
    align = open(os.path.join(CSRC, "engine_extend_align.hip")).read()
    assert "align_extend_band_fill_zdrop_kernel<K, true>" in align and "align_extend_band_fill_zdrop_kernel<K, false>" in align
    assert "&score_extend_wide_kernel<K, AFFINE, true, true, true>" in open(os.path.join(CSRC, "extend_band_align_kernels.hip.h")).read()


def test_header_states_the_definition_below_the_banded_extension_alignments():
    text = open(HEADER).read()
    decl = re.search(r"\bint\s+valign_hip_set_extend_zdrop\s*\(\s*valign_hip_engine\s*\*\s*e\s*,\s*int\s+Z\s*\)\s*;", text)
    assert decl and decl.start() > text.index("int valign_hip_set_extend_band_align(") and decl.start() < text.index("int valign_hip_host_register(")
    flat = " ".join(" ".join(re.sub(r"^\s*/?\*+\s?", "", line) for line in text.splitlines()).split())      # comment text, line frames removed
    for phrase in ("key extend_zdrop; flat API only", "\"extend_zdrop must be in [0, 2^30]\"", "Only these calls read the key", "No cell value changes",
                   "the border column counts", "it neither updates anything nor drops", "starts at the anchor (0, -1, -1)", "m_i > M: (M, Mi, Mj) = (m_i, i, c_i)",
                   "pen = (di - dj) * |ext_ref| if di > dj, else (dj - di) * |ext_read|", "the row DROPS iff M - m_i - pen > Z", "T is the first dropping row, Rp if none drops",
                   "three zeros when M = 0", "row-major first maximum over the rows < T", "gscore = VALIGN_HIP_EXTEND_UNREACHED and gref_end = 0", "Rp = 0 is five zeros",
                   "Z >= 2^29 never drops and gives the record of Z = 0 bit for bit", "M - m_i - pen lies in (-2^30, 2^29]", "BWA's ksw_extend rule",
                   "no floor at zero", "parity with BWA's numbers is not claimed", "texts that begin \"extend_zdrop:\"", "150 of its strip's 512 rows",
                   "a band of 2 * max(read_length, ref_length) is the unbanded alignment", "never picks the read end of a dropped pair",
                   "a Z-drop form of the int16 register sweep; an in-strip stop; an anti-diagonal (ksw_extz-style) rule", "\"ran_extend_zdrop\"",
                   "\"extend_zdrop_skipped_waves\"", "tests/extend_zdrop_ref.py"):
        assert phrase in flat, phrase
    # the three older sentences stand as they were, qualified by the section
    for phrase in ("NOT BUILT: Z-drop or X-drop termination -- every cell is swept", "Z-drop and a band around the anchor's diagonal remain unbuilt",
                   "NOT BUILT: Z-drop / X-drop, a band around the anchor's diagonal, the int32 route", "NOT BUILT, still: Z-drop / X-drop"):
        assert phrase in flat, phrase
    assert "The three sentences above that say \"NOT BUILT: Z-drop\" are qualified here" in flat
