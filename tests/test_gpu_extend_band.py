"""Banded extension scores (key extend_band; the BANDED instances of score_extend_wide_kernel) on the GPU, against
tests/extend_band_ref.py with B = 8 (numpy, int64 cells, the whole matrix, absent cells as a value no maximum takes; independent of
the library).  Integers, compared exactly, all five fields.

Inputs: pair k's read is random ACGT, its reference the read with d_k random bases inserted at a random position -- d_k below w
for some pairs (the band holds the path) and above w + 8 for others (it does not) -- plus trimmed tails, interior junk and a
reference cut short (an unreached read end).  Every case first asserts, on the reference alone, that some pair scores, that some
banded record differs from the unbanded one and, where the shape is meant to produce it, that some read end is unreached.

The shapes walk the windowed sweep: one strip at bands from w = 0 to the unbanded limit; two strips at the ring's and the boundary
row's 64-column blocks under a window offset, with an empty second strip, row Rp - 1 in either strip and an unreached read end;
three strips (both ping-pong slots reused: the stale columns beside each strip's window); two pairs of one wave with very different
trimmed lengths and an odd last wave."""
import functools

import numpy as np
import pytest
import torch

import extend_band_ref as ebr
import extend_ref
from test_gpu_extend import FORMS, _affine, _check, _host, _run, _scoring
from versalignlib_amd import hipkernel

pytestmark = pytest.mark.gpu

BASES = np.frombuffer(b"ACGT", np.uint8)
STRIP = 512


def _engine(R, F, sc, band_width, key=1, width=0, wide=0):
    eng = hipkernel.Engine(R, F, sc)
    eng.set_band_width(band_width)
    eng.set_extend_band(key)
    eng.set_score_width(width)
    eng.set_extend_wide(wide)
    return eng


def _ran_band(eng, n):
    d = eng.describe(0, n)
    assert d["ran_extend"] == "band" and d["ran_extend_geometry"] == "none" and d["extend_band"] == 1, (d["ran_extend"], d["ran_extend_geometry"])
    assert d["extend_band_block_rows"] == ebr.BLOCK_ROWS == hipkernel.EXTEND_BAND_BLOCK_ROWS


def _band_batch(n, R, F, band_width, seed, short_ref=True):
    """pair k: the reference is the read with d_k random bases inserted at a random position.  k % 4 == 0: d_k < max(w, 1), whole
    sequences; 1: d_k > w + 8; 2: d_k < max(w, 1) with trimmed tails (N or NUL) and an interior junk byte in both; 3: d_k = 0 and,
    short_ref, the reference cut after a few bases -- its read end lies outside every window that does not reach column -1."""
    rng = np.random.default_rng(seed)
    w = band_width // 2
    reads = BASES[rng.integers(0, 4, (n, R))]
    refs = BASES[rng.integers(0, 4, (n, F))]
    for k in range(n):
        kind = k % 4
        d = int(rng.integers(w + 9, w + 21)) if kind == 1 else (0 if kind == 3 else int(rng.integers(0, max(w, 1))))
        pos = int(rng.integers(0, max(1, min(R, F) // 2)))
        row = np.concatenate([reads[k, :pos], BASES[rng.integers(0, 4, d)], reads[k, pos:]])[:F]
        refs[k, :len(row)] = row
        if kind == 2:
            reads[k, int(rng.integers(R // 2, R + 1)):] = rng.choice([0, ord("N")])
            refs[k, int(rng.integers(F // 2, F + 1)):] = rng.choice([0, ord("N")])
            reads[k, int(rng.integers(0, max(1, R // 2)))] = ord("N")
            refs[k, int(rng.integers(0, max(1, F // 2)))] = ord("-")
        if kind == 3 and short_ref:
            refs[k, int(rng.integers(3, 9)):] = 0
    return reads, refs


def _trim_reads(reads, lengths, pairs):
    """the given pairs (none of _band_batch's trimmed kind) end at the given trimmed lengths, in turn"""
    R = reads.shape[1]
    for k, (p, Rp) in enumerate(zip(pairs, lengths)):
        assert p < len(reads) and p % 4 != 2 and 1 <= Rp <= R
        reads[p, Rp:] = ord("N") if k % 2 else 0
    return reads


def _guards(exp, free, unreached=None, differs=True):
    """on the reference alone, before the device is asked"""
    assert (exp[:, 0] > 0).any(), "no pair scores"
    if differs:
        assert (exp != free).any(), "the band changes no record"
    if unreached is not None:
        assert (exp[:, 3] == ebr.UNREACHED).any() == unreached, "an unreached read end: %s expected" % unreached
    assert ((exp[:, 3] != ebr.UNREACHED) | (exp[:, 4] == 0)).all()


# ---- 1. one strip: 33 x 70, five pairs (the last wave holds one) and one pair, bands from w = 0 to the unbanded limit ----
@pytest.mark.parametrize("band_width", [1, 2, 9, 17, 40, 400])
@pytest.mark.parametrize("form", list(FORMS))
def test_one_strip(form, band_width):
    R, F = 33, 70
    reads, refs = _band_batch(5, R, F, band_width, seed=41 + band_width)
    sc = _scoring(form)
    exp = ebr.extend(reads, refs, sc, band_width, affine=_affine(form))
    free = extend_ref.extend(reads, refs, sc, affine=_affine(form))
    limit = band_width // 2 >= max(R, F)                # w >= max(R, F): exactly the unbanded record
    _guards(exp, free, unreached=not limit, differs=not limit)
    eng = _engine(R, F, sc, band_width)
    for n in (5, 1):
        _check(_run(eng, reads[:n], refs[:n]), exp[:n], (form, band_width, n))
        _ran_band(eng, n)
    eng.close()
    if limit:
        assert np.array_equal(exp, free)
        other = hipkernel.Engine(R, F, sc)              # a second engine in the same process: the unbanded int32 sweep
        other.set_extend_wide(1)
        other.set_score_width(32)
        got = _run(other, reads, refs)
        assert other.describe(0, 5)["ran_extend"] == "wide"
        other.close()
        _check(got, exp, (form, "the unbanded sweep"))


# ---- 2. two strips: the 64-column blocks of the ring and the boundary rows under a window offset, an empty second strip
# (F <= 129), row Rp - 1 in either strip, an unreached read end ----
@pytest.mark.parametrize("band_width", [2, 16, 127, 128, 130])
@pytest.mark.parametrize("F", [63, 64, 65, 129, 600])
@pytest.mark.parametrize("R", [513, 520])
def test_two_strips(R, F, band_width):
    lengths = [100, 512, 513, R]
    reads, refs = _band_batch(9, R, F, band_width, seed=R + F + band_width, short_ref=F > 129)
    reads = _trim_reads(reads, lengths, pairs=[4, 5, 7, 8])
    Rp = extend_ref.trimmed_lengths(reads)
    assert set(lengths) <= set(Rp.tolist()) and (Rp <= STRIP).any() and (Rp > STRIP).any()
    for form in ("lin", "aff"):
        sc = _scoring(form)
        exp = ebr.extend(reads, refs, sc, band_width, affine=_affine(form), chunk=16)
        free = extend_ref.extend(reads, refs, sc, affine=_affine(form), chunk=16)
        # F <= 129: strip 1's window starts at column 512 - w >= 447, so the strip is empty and rows 512.. are unreached
        _guards(exp, free, unreached=True)
        eng = _engine(R, F, sc, band_width)
        _check(_run(eng, reads, refs), exp, (R, F, band_width, form))
        _ran_band(eng, 9)
        eng.close()


# ---- 3. three strips, both ping-pong slots reused: the columns beside each strip's window hold what strip s - 2 left there ----
@functools.lru_cache(maxsize=None)
def _three_strip_case():
    R, F, band_width = 1030, 1100, 64
    reads, refs = _band_batch(6, R, F, band_width, seed=77, short_ref=False)
    reads = _trim_reads(reads, [1030, 1025], pairs=[4, 5])
    out = {"reads": reads, "refs": refs}
    for form in ("sym", "aff"):
        out[form] = ebr.extend(reads, refs, _scoring(form), band_width, affine=_affine(form), chunk=2)
        out[form, "free"] = extend_ref.extend(reads, refs, _scoring(form), affine=_affine(form), chunk=2)
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("form", ["sym", "aff"])
def test_three_strips(form):
    case = _three_strip_case()
    _guards(case[form], case[form, "free"])
    assert (case[form][:, 1] > 2 * STRIP).any(), "no best cell in the third strip"
    eng = _engine(1030, 1100, _scoring(form), 64)
    _check(_run(eng, case["reads"].copy(), case["refs"].copy()), case[form], form)
    _ran_band(eng, 6)
    eng.close()


# ---- 4. two pairs of one wave with very different trimmed lengths, and an odd last wave ----
@pytest.mark.parametrize("band_width", [16, 130])
def test_unequal_halves_of_a_wave(band_width):
    R, F = 520, 600
    reads, refs = _band_batch(12, R, F, band_width, seed=5 + band_width, short_ref=False)
    reads, refs = reads[::4].copy(), refs[::4].copy()   # three pairs of whole sequences with few inserted bases
    refs[0, :R] = reads[0]                             # pair 0: the whole read on the diagonal, both sequences whole
    reads[1, 20:] = 0                                   # pair 1, the same wave: Rp = 20, Fp = 30
    refs[1, 30:] = ord("N")
    reads[2, 515:] = ord("N")                           # pair 2, alone in the last wave; its reference ends before strip 1's window
    refs[2, 300:] = 0
    Rp, Fp = extend_ref.trimmed_lengths(reads), extend_ref.trimmed_lengths(refs)
    assert Rp.tolist() == [520, 20, 515] and Fp.tolist() == [600, 30, 300]
    for form in ("lin", "affsym"):
        sc = _scoring(form)
        exp = ebr.extend(reads, refs, sc, band_width, affine=_affine(form))
        free = extend_ref.extend(reads, refs, sc, affine=_affine(form))
        _guards(exp, free, unreached=True)
        assert exp[0, 0] == 2 * R and exp[2, 3] == ebr.UNREACHED and exp[1, 3] != ebr.UNREACHED
        eng = _engine(R, F, sc, band_width)
        for n in (3, 2, 1):
            _check(_run(eng, reads[:n], refs[:n]), exp[:n], (band_width, form, n))
        got = _run(eng, reads[::-1].copy(), refs[::-1].copy())           # the pairs change halves and waves
        _check(got, exp[::-1], (band_width, form, "reversed"))
        eng.close()


# ---- 5. score_width 0 and 32, extend_wide 0 and 1: the same records on the same route; short reads too ----
def test_score_width_and_extend_wide_change_nothing():
    R, F, band_width = 150, 300, 24
    reads, refs = _band_batch(8, R, F, band_width, seed=12)
    sc = _scoring("aff")
    exp = ebr.extend(reads, refs, sc, band_width, affine=True)
    _guards(exp, extend_ref.extend(reads, refs, sc, affine=True), unreached=True)
    for width in (0, 32):
        for wide in (0, 1):
            eng = _engine(R, F, sc, band_width, width=width, wide=wide)
            _check(_run(eng, reads, refs), exp, (width, wide))
            _ran_band(eng, 8)
            eng.close()


# ---- 6. the host entry: the chunk pipeline on one stream equals the device entry ----
def test_host_entry():
    R, F, band_width, n = 520, 600, 40, 37
    reads, refs = _band_batch(n, R, F, band_width, seed=6)
    sc = _scoring("affsym")
    exp = ebr.extend(reads, refs, sc, band_width, affine=True, chunk=16)
    _guards(exp, extend_ref.extend(reads, refs, sc, affine=True, chunk=16), unreached=True)
    eng = _engine(R, F, sc, band_width)
    dev = _run(eng, reads, refs)
    _check(dev, exp, "device")
    for threads in (1, 3):
        _check(_host(eng, reads, refs, threads), dev, ("host", threads))
        _ran_band(eng, n)
    eng.close()


# ---- 7. refusals, each with its text and "ran_extend": "none" ----
def test_refusals():
    R, F = 33, 70
    reads, refs = _band_batch(4, R, F, 16, seed=3)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()

    def refused(eng, word, opt=0, rd=d_reads, rf=d_refs, host=(reads, refs)):
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.score_extend_device(opt, rd, rf)
        assert eng.describe(0, 4)["ran_extend"] == "none"
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.score_extend_host(opt, host[0], host[1])
        assert eng.describe(0, 4)["ran_extend"] == "none"

    sc = _scoring("sym")
    eng = _engine(R, F, sc, 16)
    exp = ebr.extend(reads, refs, sc, 16)
    _check(_run(eng, reads, refs), exp, "before the refusals")
    _ran_band(eng, 4)
    refused(eng, "opt & 0xF == 0 only", opt=1)
    eng.set_traceback_policy(1)
    refused(eng, "traceback_policy = 1")
    eng.set_traceback_policy(0)
    eng.set_score_width(16)
    refused(eng, "^extend_band: .*score_width = 16")
    eng.set_score_width(0)
    with pytest.raises(hipkernel.HipKernelError, match="extend_band must be 0 or 1"):
        eng.set_extend_band(2)
    assert eng.describe(0, 4)["extend_band"] == 1
    # extension alignments under a band: a text of their own with the key on, the scores' text with the key off
    for call in (lambda: eng.align_extend_device(0, d_reads, d_refs), lambda: eng.align_extend_host(0, reads, refs)):
        with pytest.raises(hipkernel.HipKernelError, match="^extension alignments: not built under a band"):
            call()
        assert eng.describe(0, 4)["ran_extend_align"] == "none"
        eng.set_extend_band(0)
        with pytest.raises(hipkernel.HipKernelError, match="extension scores are not built for band_width > 0"):
            call()
        eng.set_extend_band(1)
    # key off: today's text
    eng.set_extend_band(0)
    refused(eng, "extension scores are not built for band_width > 0")
    eng.set_extend_band(1)
    _check(_run(eng, reads, refs), exp, "after the refusals")
    eng.close()
    # the band's int32 bound: 10 000 gap steps at -30 000 (the refusal comes before anything is launched)
    big = np.full((2, 5000), ord("A"), np.uint8)
    eng = _engine(5000, 5000, hipkernel.Scoring.make(2, -1, -30000, -30000), 64)
    refused(eng, "^extend_band: shape x scoring", rd=torch.from_numpy(big).cuda(), rf=torch.from_numpy(big).cuda(), host=(big, big))
    eng.close()


# ---- 8. the key: not read without a band, not read by placed scores, and cleared again ----
def test_key_behaviour():
    R, F = 150, 300
    reads, refs = _band_batch(6, R, F, 24, seed=8)
    sc = _scoring("lin")
    free = extend_ref.extend(reads, refs, sc)
    banded = ebr.extend(reads, refs, sc, 24)
    _guards(banded, free, unreached=True)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    eng = hipkernel.Engine(R, F, sc)
    placed = eng.score_placed_device(0, d_reads, d_refs).cpu().numpy()
    assert eng.describe(0, 6)["extend_band"] == 0
    # band_width = 0: the key changes nothing
    _check(_run(eng, reads, refs), free, "key off, no band")
    eng.set_extend_band(1)
    _check(_run(eng, reads, refs), free, "key on, no band")
    d = eng.describe(0, 6)
    assert d["ran_extend"] == "rows" and d["extend_band"] == 1
    # placed scores on the same engine do not read it
    assert np.array_equal(eng.score_placed_device(0, d_reads, d_refs).cpu().numpy(), placed)
    # the band and the key ...
    eng.set_band_width(24)
    _check(_run(eng, reads, refs), banded, "band and key")
    _ran_band(eng, 6)
    # ... then both cleared: the unbanded records again
    eng.set_band_width(0)
    eng.set_extend_band(0)
    _check(_run(eng, reads, refs), free, "both cleared")
    assert eng.describe(0, 6)["ran_extend"] == "rows"
    assert np.array_equal(eng.score_placed_device(0, d_reads, d_refs).cpu().numpy(), placed)
    eng.close()
