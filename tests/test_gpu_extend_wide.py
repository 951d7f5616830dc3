"""Extension scores on int32 cells and row strips (key extend_wide; score_extend_wide_kernel) on the GPU, against
tests/extend_ref.py (numpy, int64 cells, the whole matrix, independent of the library).  Integers, compared exactly, all five
fields.  The shapes walk the sweep's paths: one strip with padding rows below the read, two strips at the ring's and the boundary
row's 64-column blocks with row Rp - 1 in either strip, three strips (both ping-pong slots reused), a last wave of one pair."""
import functools

import numpy as np
import pytest
import torch

import extend_ref
from conftest import debug_switches
from test_gpu_extend import FORMS, _affine, _batch, _check, _host, _run, _scoring
from versalignlib_amd import hipkernel

pytestmark = pytest.mark.gpu

STRIP = 512          # rows of a strip: 64 lanes x 8 rows


def _engine(R, F, sc, width=32, wide=1):
    eng = hipkernel.Engine(R, F, sc)
    eng.set_extend_wide(wide)
    eng.set_score_width(width)
    return eng


def _ran_wide(eng, n):
    d = eng.describe(0, n)
    assert d["ran_extend"] == "wide" and d["ran_extend_geometry"] == "none" and d["extend_wide"] == 1, (d["ran_extend"], d["ran_extend_geometry"])


def _trim_reads(reads, lengths):
    """the odd pairs (_batch trims the even ones at random) end at the given trimmed lengths, in turn"""
    R = reads.shape[1]
    for k, Rp in enumerate(lengths):
        p = 2 * k + 1
        assert p < len(reads) and 1 <= Rp <= R
        reads[p, Rp:] = ord("N") if k % 2 else 0
    return reads


# ---- 1. one strip: 33 x 70 under score_width = 32, five pairs (the last wave holds one) and one pair ----
@pytest.mark.parametrize("form", list(FORMS))
def test_one_strip(form):
    R, F = 33, 70
    reads, refs = _batch(5, R, F, seed=41)
    sc = _scoring(form)
    exp = extend_ref.extend(reads, refs, sc, affine=_affine(form))
    eng = _engine(R, F, sc)
    for n in (5, 1):
        _check(_run(eng, reads[:n], refs[:n]), exp[:n], (form, n))
        _ran_wide(eng, n)
    eng.close()
    assert (exp[:, 0] > 0).any()


# ---- 2. two strips: the ring's and the boundary row's 64-column blocks, row Rp - 1 in strip 0 and in strip 1 ----
@pytest.mark.parametrize("F", [63, 64, 65, 129, 300])
@pytest.mark.parametrize("R", [513, 520])
def test_two_strips(R, F):
    lengths = [100, 512, 513, R]
    reads, refs = _batch(9, R, F, seed=R + F)
    reads = _trim_reads(reads, lengths)
    Rp = extend_ref.trimmed_lengths(reads)
    assert set(lengths) <= set(Rp.tolist()) and (Rp <= STRIP).any() and (Rp > STRIP).any()
    for form in FORMS:
        sc = _scoring(form)
        exp = extend_ref.extend(reads, refs, sc, affine=_affine(form), chunk=16)
        eng = _engine(R, F, sc)
        _check(_run(eng, reads, refs), exp, (R, F, form))
        _ran_wide(eng, 9)
        eng.close()


# ---- 3. three strips, both ping-pong slots reused: by the read's length alone (score_width = 0) and under score_width = 32 ----
@functools.lru_cache(maxsize=None)
def _three_strip_case():
    R, F = 1030, 200
    reads, refs = _batch(6, R, F, seed=77)
    reads = _trim_reads(reads, [1030, 1025, 700])
    out = {"reads": reads, "refs": refs}
    for form in FORMS:
        out[form] = extend_ref.extend(reads, refs, _scoring(form), affine=_affine(form), chunk=8)
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("width", [0, 32])
@pytest.mark.parametrize("form", list(FORMS))
def test_three_strips(form, width):
    case = _three_strip_case()
    eng = _engine(1030, 200, _scoring(form), width=width)
    _check(_run(eng, case["reads"].copy(), case["refs"].copy()), case[form], (form, width))
    _ran_wide(eng, 6)
    eng.close()


# ---- 4. values that need int32: the scorings the int16 route refuses (tests/test_gpu_extend.py::test_refusals) ----
@pytest.mark.parametrize("match", [970, 1000])
def test_score_above_int16(match):
    """33 x 970 = 32010 is beyond the +-32000 the int16 rule allows (the scoring test_refusals refuses); 33 x 1000 is beyond int16"""
    R, F = 33, 70
    reads, refs = _batch(4, R, F, seed=3, trim=False)
    refs[0, :R] = reads[0]                  # an identical 33-base prefix
    sc = hipkernel.Scoring.make(match, -1, -3, -3)
    exp = extend_ref.extend(reads, refs, sc)
    assert exp[0, 0] == 33 * match > 32000 and exp[0, 1] == 33 and exp[0, 2] == 33 and (match == 970 or exp[0, 0] > 32767)
    eng = _engine(R, F, sc, width=0)
    _check(_run(eng, reads, refs), exp, ("match", match))
    _ran_wide(eng, 4)
    eng.close()


def test_border_column_below_int16():
    R, F = 120, 70
    reads, refs = _batch(3, R, F, seed=5, trim=False)
    refs[1, :] = ord("N")                   # no ACGT byte: nothing but the border column
    sc = hipkernel.Scoring.make(2, -1, -320, -320)
    exp = extend_ref.extend(reads, refs, sc)
    assert exp[1].tolist() == [0, 0, 0, -38400, 0]
    eng = _engine(R, F, sc, width=0)
    _check(_run(eng, reads, refs), exp, "gaps of -320")
    _ran_wide(eng, 3)
    eng.close()


# ---- 5. ties across strips: the maximum stands in strip 0 and in strip 1, the record's end cell is the row-major first one ----
@pytest.mark.parametrize("form", ["sym", "affsym"])
def test_ties_across_strips(form):
    R, F = 520, 530
    rng = np.random.default_rng(8)
    two = np.frombuffer(b"AC", np.uint8)
    reads, refs = two[rng.integers(0, 2, (4, R))], two[rng.integers(0, 2, (4, F))]
    # pairs 0 and 1: 510 matches, then mismatch / match twice -- 1020 at rows 509, 511 (strip 0) and 513 (strip 1) -- then no match
    for p in (0, 1):
        refs[p, :510] = reads[p, :510]
        for i in (510, 512):
            reads[p, i], refs[p, i] = ord("A"), ord("C")
            reads[p, i + 1] = refs[p, i + 1] = ord("A")
        reads[p, 514:], refs[p, 514:] = ord("A"), ord("C")
    sc = hipkernel.Scoring.make(2, -2, *FORMS[form])
    X = extend_ref.matrices(reads, refs, sc, affine=_affine(form))[:, 1:, 1:]
    tied = 0
    for p in range(4):
        rows = np.nonzero((X[p] == X[p].max()).any(axis=1))[0]
        tied += int(X[p].max() > 0 and rows.min() < STRIP <= rows.max())
    assert tied >= 1
    exp = extend_ref.extend(reads, refs, sc, affine=_affine(form))
    assert exp[0, :3].tolist() == [1020, 510, 510]
    eng = _engine(R, F, sc)
    _check(_run(eng, reads, refs), exp, form)
    _ran_wide(eng, 4)
    eng.close()


# ---- 6. the same records on both routes, inside the int16 range ----
@pytest.mark.parametrize("R,F", [(150, 300), (500, 700)])
def test_equals_the_rows_route_in_range(R, F):
    n = 33
    reads, refs = _batch(n, R, F, seed=R)
    for form in ("lin", "aff"):
        eng = _engine(R, F, _scoring(form))
        wide = _run(eng, reads, refs)
        _ran_wide(eng, n)
        eng.set_extend_wide(0)
        eng.set_score_width(0)
        rows = _run(eng, reads, refs)
        assert eng.describe(0, n)["ran_extend"] == "rows"
        eng.close()
        _check(wide, rows, (R, F, form))
    _check(wide[:8], extend_ref.extend(reads[:8], refs[:8], _scoring("aff"), affine=True, chunk=8), "against the reference")


# ---- 7. the empty cases ----
def test_empty_cases():
    R, F = 33, 70
    reads, refs = _batch(6, R, F, seed=13, trim=False)
    reads[1, :] = ord("N")                              # no ACGT byte in the read: five zeros
    reads[2, :] = 0
    reads[3, :], refs[3, :] = ord("A"), ord("C")        # no positive cell: three zeros, gscore still reported
    for form in ("lin", "affsym"):
        sc = _scoring(form)
        exp = extend_ref.extend(reads, refs, sc, affine=_affine(form))
        assert exp[1].tolist() == [0] * 5 and exp[2].tolist() == [0] * 5 and exp[3, :3].tolist() == [0, 0, 0] and exp[3, 3] < 0
        eng = _engine(R, F, sc)
        _check(_run(eng, reads, refs), exp, form)
        eng.close()


# ---- 8. the host path: the chunk pipeline (several chunks, 4-bit classes and raw ASCII, the direct call) equals the device path ----
@pytest.mark.parametrize("chunks", [False, True])
def test_host_path_equals_device_path(monkeypatch, chunks):
    if chunks:
        debug_switches(monkeypatch, chunk_bytes=200000)
    R, F, n = 64, 128, 5000
    reads, refs = _batch(n, R, F, seed=12)
    for form in ("lin", "affsym"):
        eng = _engine(R, F, _scoring(form))
        dev = _run(eng, reads, refs)
        for threads in (1, 4):
            _check(_host(eng, reads, refs, threads), dev, (form, threads, chunks))
        _ran_wide(eng, n)
        assert eng.describe(0, n)["direct_call"] == 0
        eng.set_host_packing(0)
        _check(_host(eng, reads, refs, 2), dev, (form, "raw ASCII", chunks))
        _check(_host(eng, reads[:100], refs[:100], 2), dev[:100], (form, "direct"))
        eng.close()
    _check(dev[:256], extend_ref.extend(reads[:256], refs[:256], _scoring("affsym"), affine=True), "device path")


# ... the int32 placed sweep and the extension sweep share the engine's scratch: either order, either size
def test_placed_and_extension_sweeps_share_one_engine():
    R, F, n = 600, 90, 67
    reads, refs = _batch(n, R, F, seed=21)
    sc = _scoring("aff")
    exp = extend_ref.extend(reads, refs, sc, affine=True, chunk=16)
    eng = _engine(R, F, sc)
    eng.set_placed_wide(1)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    _check(_run(eng, reads, refs), exp, "first")
    placed = eng.score_placed_device(0, d_reads, d_refs)
    torch.cuda.synchronize()
    _check(_run(eng, reads[:21], refs[:21]), exp[:21], "after a placed call, fewer pairs")
    placed_again = eng.score_placed_device(0, d_reads, d_refs)
    torch.cuda.synchronize()
    _check(_run(eng, reads, refs), exp, "after a second placed call")
    eng.close()
    assert np.array_equal(placed.cpu().numpy(), placed_again.cpu().numpy()) and (placed.cpu().numpy()[:, 0].astype(np.int64) >= exp[:, 0]).all()


# ... and the strip sweep cut into several scratch chunks, the last one short with a last wave of one pair
def test_sweep_in_several_scratch_chunks():
    R, F, n = 1025, 700, 151             # the capped shape of tests/test_gpu_placed_wide.py: chunks of 72 pairs under 1 MiB, 151 = 2 x 72 + 7
    reads, refs = _batch(n, R, F, seed=1616)
    sc = _scoring("aff")
    eng = _engine(R, F, sc, width=0)
    whole = _run(eng, reads, refs)
    eng.close()
    eng = _engine(R, F, sc, width=0)
    eng.set_pointer_scratch_cap_mb(1)
    capped = _run(eng, reads, refs)
    _ran_wide(eng, n)
    host = _host(eng, reads, refs, 2)
    eng.close()
    _check(capped, whole, "capped against uncapped")
    _check(host, whole, "capped host path")
    _check(capped[:6], extend_ref.extend(reads[:6], refs[:6], sc, affine=True, chunk=6), "against the reference")


# ---- 9. the key, the refusals that stay, describe() ----
def test_key_refusals_and_describe():
    R, F = 33, 70
    reads, refs = _batch(4, R, F, seed=3)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    sc = _scoring("sym")
    exp = extend_ref.extend(reads, refs, sc)

    def refused(eng, word, opt=0, rd=d_reads, rf=d_refs, host=(reads, refs)):
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.score_extend_device(opt, rd, rf)
        assert eng.describe(0, 4)["ran_extend"] == "none"
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.score_extend_host(opt, host[0], host[1])
        assert eng.describe(0, 4)["ran_extend"] == "none"

    eng = hipkernel.Engine(R, F, sc)
    assert eng.describe(0, 4)["extend_wide"] == 0
    for bad in (2, -1):
        with pytest.raises(hipkernel.HipKernelError, match="extend_wide must be 0 or 1"):
            eng.set_extend_wide(bad)
    eng.set_extend_wide(1)
    # the register sweep serves the call: it keeps it
    _check(_run(eng, reads, refs), exp, "in range, key on")
    assert eng.describe(0, 4)["ran_extend"] == "rows" and eng.describe(0, 4)["ran_extend_geometry"] != "none"
    eng.set_score_width(32)
    _check(_run(eng, reads, refs), exp, "score_width = 32")
    _ran_wide(eng, 4)
    refused(eng, "opt & 0xF == 0 only", opt=1)
    out = torch.full((4, 5), -7, dtype=torch.int32, device="cuda")          # opt & 0xF > 1 does nothing
    eng.score_extend_device(2, d_reads, d_refs, out=out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all()
    eng.set_traceback_policy(1)
    refused(eng, "traceback_policy = 1")
    eng.set_traceback_policy(0)
    for band_placed in (0, 1):
        eng.set_band_placed(band_placed)
        eng.set_band_width(16)
        refused(eng, "not built for band_width > 0")
        eng.set_band_width(0)
    eng.set_band_placed(0)
    _check(_run(eng, reads, refs), exp, "after the refusals")
    _ran_wide(eng, 4)
    # the key off again: the same engine refuses as before and runs rows where it did
    eng.set_extend_wide(0)
    for placed_wide in (0, 1):
        eng.set_placed_wide(placed_wide)
        refused(eng, "not built for score_width = 32")
    eng.set_placed_wide(0)
    eng.set_score_width(0)
    _check(_run(eng, reads, refs), exp, "key off")
    assert eng.describe(0, 4)["ran_extend"] == "rows" and eng.describe(0, 4)["extend_wide"] == 0
    eng.close()
    # out of the int16 range: score_width = 16 stays refused with the key on, 0 runs wide, the key off refuses as ever
    for scoring in (hipkernel.Scoring.make(970, -1, -3, -3), hipkernel.Scoring.make(2, -1, -320, -320)):
        eng = hipkernel.Engine(R, F, scoring)
        refused(eng, "signed int16 cells")
        eng.set_extend_wide(1)
        eng.set_score_width(16)
        refused(eng, "signed int16 cells")
        eng.set_score_width(0)
        _check(_run(eng, reads, refs), extend_ref.extend(reads, refs, scoring), "out of range, key on")
        _ran_wide(eng, 4)
        eng.set_extend_wide(0)
        refused(eng, "signed int16 cells")
        eng.close()
    # the row strips' shapes: refused without the key
    big = np.full((2, 1500), ord("A"), np.uint8)
    d_big = torch.from_numpy(big).cuda()
    eng = hipkernel.Engine(1500, 1500, sc)
    refused(eng, "register sweep only", rd=d_big, rf=d_big, host=(big, big))
    eng.close()
    # beyond extend_int32_ok: 10 000 gap steps at -30 000 pass -2^28
    deep = np.full((2, 5000), ord("A"), np.uint8)
    d_deep = torch.from_numpy(deep).cuda()
    eng = hipkernel.Engine(5000, 5000, hipkernel.Scoring.make(2, -1, -30000, -30000))
    eng.set_extend_wide(1)
    refused(eng, "extend_wide: shape x scoring", rd=d_deep, rf=d_deep, host=(deep, deep))
    eng.close()
