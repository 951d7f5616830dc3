"""Extension Z-drop (key extend_zdrop; the ZDROP instances of score_extend_wide_kernel) on the GPU, against
tests/extend_zdrop_ref.py (numpy / plain Python, int64 cells, the whole matrix, the row loop of the definition; independent of the
library).  Integers, compared exactly: all five fields of every record, the count of skipped waves, and for alignments records,
ops and extension records.

Inputs are planted: pair k's reference is the read's first a_k bases, then g bases of C where the read holds A, then the read's
continuation -- the first drop falls a few rows behind a_k and the unbounded record reaches into the second segment.  Where a
case needs a drop row T exactly, a_k is searched among the 14 values up to T, on the reference.  Every case first asserts, on the
reference alone (_guards), that some pair scores, that some record differs from the one without the key, that the listed drop rows
occur and that the expected count of skipped waves is what the case is meant to show."""
import functools

import numpy as np
import pytest
import torch

import extend_band_align_ref as ebar
import extend_band_ref as ebr
import extend_ref
import extend_zdrop_ref as ezr
from test_gpu_extend import FORMS, _affine, _check, _host, _run, _scoring
from test_gpu_extend_align import _run as _run_align
from versalignlib_amd import hipkernel

pytestmark = pytest.mark.gpu

BASES = np.frombuffer(b"ACGT", np.uint8)
STRIP = 512
NEVER = 1 << 29
GAP = 14                        # g: rows of A against C, enough for a drop under Z = 30 at a mismatch of -3

TEXT_NO_INT16 = "extend_zdrop: Z-dropped extension scores run on int32 cells; score_width = 16 (int16 or refuse) is refused"
TEXT_ALIGN = ("extend_zdrop: Z-dropped extension alignments run on the banded route only (band_width > 0 with extend_band = 1 and "
              "extend_band_align = 1); a band of 2 * max(read_length, ref_length) is the unbanded alignment")
TEXT_KEY = "extend_zdrop must be in [0, 2^30]"


def _sc(form):
    return _scoring(form, 2, -3)


def _engine(R, F, sc, Z, band_width=0, align=0):
    eng = hipkernel.Engine(R, F, sc)
    eng.set_band_width(band_width)
    eng.set_extend_band(1 if band_width else 0)
    eng.set_extend_band_align(align)
    eng.set_extend_zdrop(Z)
    return eng


def _plant(base, F, a, g=GAP):
    """-> read, ref: the read is `base` with g bases of A from a on; the reference follows it except for g bases of C there"""
    R = len(base)
    read = base.copy()
    read[a:a + g] = ord("A")
    ref = np.full(F, ord("T"), np.uint8)
    m = min(R, F)
    ref[:m] = read[:m]
    ref[a:min(a + g, F)] = ord("C")
    return read, ref


def _plant_at(rng, R, F, sc, affine, Z, band_width, T, window=14, tries=1):
    """a pair whose first dropping row is T: a_k searched among the `window` values up to T, one batch on the reference per random
    read.  (Under Z = 10 and the linear gaps -2 / -4 the drop falls 3 rows behind a_k; where a gap is as cheap as a mismatch, or
    affine, the penalty pays for the gap and the drop falls later, by an amount that depends on the sequences.)"""
    for _ in range(tries):
        base = BASES[rng.integers(0, 4, R)]
        starts = list(range(max(1, T - window + 1), T + 1))
        pairs = [_plant(base, F, a) for a in starts]
        reads, refs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        # (the first drop at row T < R is decided by the rows up to T: the reference sees no more of the reads)
        _, rows = ezr.extend(reads[:, :T + 1] if T < R else reads, refs, sc, Z, band_width, affine, chunk=len(starts))
        hit = np.nonzero(rows == T)[0]
        if hit.size:
            return reads[hit[0]], refs[hit[0]]
    raise AssertionError(("no a_k drops at row", T, rows.tolist()))


def _whole(rng, R, F):
    """a pair that never drops: the reference follows the read to its end"""
    read = BASES[rng.integers(0, 4, R)]
    ref = BASES[rng.integers(0, 4, F)]
    ref[:min(R, F)] = read[:min(R, F)]
    return read, ref


def _guards(exp, T, free, Rp, rows=(), undropped=True):
    assert (exp[:, 0] > 0).any(), "no pair scores"
    assert (exp != free).any(), "the key changes no record"
    assert set(rows) <= set(T[T < Rp].tolist()), ("drop rows", rows, T.tolist())
    if undropped:
        assert (T == Rp).any(), "no pair runs to its end"
    assert ((T == Rp) | ((exp[:, 3] == ezr.UNREACHED) & (exp[:, 4] == 0))).all()


def _ran(eng, n, Z, route, skipped=None):
    d = eng.describe(0, n)
    assert d["ran_extend"] == route and d["extend_zdrop"] == Z and d["ran_extend_zdrop"] == Z, (d["ran_extend"], d["extend_zdrop"], d["ran_extend_zdrop"])
    if skipped is not None:
        assert d["extend_zdrop_skipped_waves"] == skipped, (d["extend_zdrop_skipped_waves"], skipped)
    return d


def _free(reads, refs, sc, band_width, affine, chunk=16):
    return ebr.extend(reads, refs, sc, band_width, affine, chunk=chunk) if band_width else extend_ref.extend(reads, refs, sc, affine, chunk=chunk)


# ---- 1. one strip: 33 x 70, five pairs (the last wave holds one) and one pair; drops at a lane's last and first row ----
# Which rows can drop depends on the gap form.  With the linear gaps -2 / -4 a drop under Z needs ceil((Z + 1) / 3) mismatching rows
# behind a best of at least that: rows 7 and 8 up to Z = 10, 15 and 16 at 30, asserted literally.  Where a gap is as cheap as a
# mismatch, or affine, the gap path from the best cell is the row's maximum and the penalty pays for it: the drop falls later, if at
# all -- so the pairs are chosen from the drop rows of every a_k, on the reference: a lane's last row and a lane's first row where
# they occur, and other rows.
def _edge_rows(Z):
    return (7, 8) if Z <= 10 else (15, 16)


def _one_strip_pairs(rng, R, F, sc, affine, Z, band_width):
    """-> reads, refs of five pairs (the fourth never drops), and whether any a_k drops at all"""
    literal = Z < NEVER and not affine and sc.gap_read != sc.gap_ref
    for _ in range(8):      # (a random read whose bases beside the planted run shift a drop row is drawn again)
        base = BASES[rng.integers(0, 4, R)]
        starts = list(range(1, R - 1))
        table = [_plant(base, F, a) for a in starts]
        _, rows = ezr.extend(np.stack([p[0] for p in table]), np.stack([p[1] for p in table]), sc, Z, band_width, affine, chunk=len(starts))
        first = {}
        for k, T in enumerate(rows.tolist()):
            if T < R:
                first.setdefault(T, k)
        if not literal or set(_edge_rows(Z)) <= set(first):
            break
    order = [T for T in first if T % 8 == 7][:1] + [T for T in first if T % 8 == 0][:1]
    if literal:
        order = list(_edge_rows(Z))
    order += [T for T in sorted(first) if T not in order]
    picks = [first[T] for T in order[:4]] + [3, 9, 14, 20][len(order[:4]):]
    pairs = [table[k] for k in picks[:3]] + [_whole(rng, R, F), table[picks[3]]]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), bool(first)


@pytest.mark.parametrize("band_width", [0, 9, 40, 400])
@pytest.mark.parametrize("Z", [1, 10, 30, NEVER])
@pytest.mark.parametrize("form", list(FORMS))
def test_one_strip(form, Z, band_width):
    R, F = 33, 70
    sc, affine = _sc(form), _affine(form)
    rng = np.random.default_rng(7 * Z % 1000 + band_width)
    reads, refs, drops = _one_strip_pairs(rng, R, F, sc, affine, Z, band_width)
    exp, T = ezr.extend(reads, refs, sc, Z, band_width, affine)
    free = _free(reads, refs, sc, band_width, affine)
    Rp = extend_ref.trimmed_lengths(reads)
    if drops:
        _guards(exp, T, free, Rp, rows=_edge_rows(Z) if form == "lin" else ())
    else:                   # Z = 2^29, and the affine forms under Z = 30 without a band: no a_k drops within 33 rows
        assert (Z == NEVER or (affine and Z == 30)) and np.array_equal(exp, free) and (T == Rp).all() and (exp[:, 0] > 0).any()
    eng = _engine(R, F, sc, Z, band_width)
    for n in (5, 1):
        _check(_run(eng, reads[:n], refs[:n]), exp[:n], (form, Z, band_width, n))
        _ran(eng, n, Z, "band" if band_width else "wide", skipped=0)
    eng.close()
    if Z == NEVER:          # a second engine with the key off: the same records
        other = _engine(R, F, sc, 0, band_width)
        if not band_width:
            other.set_extend_wide(1)
            other.set_score_width(32)
        _check(_run(other, reads, refs), exp, (form, band_width, "the key off"))
        assert other.describe(0, 5)["ran_extend_zdrop"] == 0
        other.close()


# ---- 2. two strips: drops at the strip's edge, a pair that ends there, a wave that skips and a wave of a dropped and an undropped pair ----
@functools.lru_cache(maxsize=None)
def _two_strip_case(R, F, form, band_width, Z=10):
    sc, affine = _sc(form), _affine(form)
    rng = np.random.default_rng(R + F + band_width)
    at = lambda T: _plant_at(rng, R, F, sc, affine, Z, band_width, T)
    if form != "lin":       # drop rows as they fall (see _edge_rows): the drops of strip 0, the waves as below
        at = lambda T: _plant(BASES[rng.integers(0, 4, R)], F, max(1, T - 40))
    if F >= R:
        rows = (100, 511, 512) + ((513,) if R > 514 else ())
        ends = list(_whole(rng, R, F))
        ends[0][STRIP:] = ord("N")                      # Rp = 512, no drop
        #        wave 0: skips       wave 1: T = 512 runs    wave 2: undropped + dropped    wave 3                            wave 4: alone, skips
        pairs = [at(100), at(511), at(512), at(100), tuple(ends), at(100), at(513 if R > 514 else 100), _whole(rng, R, F), at(100)]
        skipped = 2 if form == "lin" else None
    else:                   # a short reference: the homology ends with it, every drop lies in strip 0
        rows = (20, 40)
        pairs = [at(20), at(40), at(20), _whole(rng, R, F), at(40)]
        skipped = 0 if band_width else 2                # (under the band strip 1's window starts beyond the reference: it returns as empty)
    reads, refs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    exp, T = ezr.extend(reads, refs, sc, Z, band_width, affine, chunk=3)
    free = _free(reads, refs, sc, band_width, affine, chunk=3)
    Rp, Fp = extend_ref.trimmed_lengths(reads), extend_ref.trimmed_lengths(refs)
    _guards(exp, T, free, Rp, rows=rows if form == "lin" else ())
    count = ezr.skipped_waves(T, Rp, Fp, R, band_width)
    if skipped is None:
        skipped = count
        assert (T[[0, 1, 8]] < STRIP).all() and count >= 2, (count, T.tolist())
    assert count == skipped and (skipped > 0 or (band_width and F < R)), (count, skipped, T.tolist())
    if F >= R:
        assert Rp[4] == STRIP and T[4] == STRIP and T[5] < STRIP          # the wave of an undropped and a dropped pair
    for a in (reads, refs, exp, T):
        a.setflags(write=False)
    return reads, refs, exp, T, count


@pytest.mark.parametrize("band_width", [0, 130])
@pytest.mark.parametrize("form", ["lin", "aff"])
@pytest.mark.parametrize("F", [65, 600])
@pytest.mark.parametrize("R", [513, 520])
def test_two_strips(R, F, form, band_width):
    reads, refs, exp, T, count = _two_strip_case(R, F, form, band_width)
    eng = _engine(R, F, _sc(form), 10, band_width)
    _check(_run(eng, reads.copy(), refs.copy()), exp, (R, F, form, band_width))
    _ran(eng, len(reads), 10, "band" if band_width else "wide", skipped=count)
    eng.close()


# ---- 3. three strips: a drop in strip 0 skips two strips; a pair that never scores and still drops; an odd last wave ----
@functools.lru_cache(maxsize=None)
def _three_strip_case(form, band_width, Z=10):
    R, F = 1030, 1100
    sc, affine = _sc(form), _affine(form)
    rng = np.random.default_rng(31 + band_width)
    base = lambda: BASES[rng.integers(0, 4, R)]
    never = (np.full(R, ord("A"), np.uint8), np.full(F, ord("C"), np.uint8))           # M = 0 throughout, and it drops
    pairs = [_plant(base(), F, 50), _plant(base(), F, 200), never, _plant(base(), F, 300), _whole(rng, R, F), _plant(base(), F, 120), _plant(base(), F, 400)]
    reads, refs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    exp, T = ezr.extend(reads, refs, sc, Z, band_width, affine, chunk=4)
    free = _free(reads, refs, sc, band_width, affine, chunk=4)
    Rp, Fp = extend_ref.trimmed_lengths(reads), extend_ref.trimmed_lengths(refs)
    _guards(exp, T, free, Rp)
    # all A against all C never scores.  It drops where the row's maximum is a cell the penalty does not pay for: on the diagonal
    # under the gaps -2 / -4, and under a band once the border column has left it; unbanded under the affine form it never drops
    if form == "lin" or band_width:
        assert exp[2].tolist() == [0, 0, 0, ezr.UNREACHED, 0] and T[2] < STRIP
    else:
        assert exp[2, :3].tolist() == [0, 0, 0] and T[2] == R
    assert (T[[0, 1, 3, 5, 6]] < STRIP).all() and T[4] == R
    count = ezr.skipped_waves(T, Rp, Fp, R, band_width)
    # waves (0, 1) and (6) skip both strips, (4, 5) runs; (2, 3) skips both where its first pair drops
    assert count == 2 + (2 if T[2] < STRIP else 0) + 0 + 2, count
    for a in (reads, refs, exp):
        a.setflags(write=False)
    return reads, refs, exp, count


@pytest.mark.parametrize("band_width", [0, 16, 130])
@pytest.mark.parametrize("form", ["lin", "aff"])
def test_three_strips(form, band_width):
    reads, refs, exp, count = _three_strip_case(form, band_width)
    eng = _engine(1030, 1100, _sc(form), 10, band_width)
    _check(_run(eng, reads.copy(), refs.copy()), exp, (form, band_width))
    _ran(eng, 7, 10, "band" if band_width else "wide", skipped=count)
    eng.close()


# ---- 4. alignments under the band: the alignment of the pair cut to its first T rows, never from a dropped pair's read end ----
def _align_expect(reads, refs, sc, affine, band_width, T, Rp, bonus, zrecords):
    cut = ezr.cut_reads(reads, T)
    best, chosen = ebar.align(cut, refs, sc, band_width, affine, end_bonus=(-1, bonus), chunk=3)
    dropped = T < Rp
    recs = np.where(dropped[:, None], best[0], chosen[0])
    ops = [best[1][k] if dropped[k] else chosen[1][k] for k in range(len(reads))]
    for k in np.nonzero(dropped)[0]:                    # the read end is never chosen where T < Rp
        assert recs[k, 1] <= T[k] and recs[k, 1] == zrecords[k, 1]
    return recs, ops, zrecords, None


def _check_align(got, exp, what):
    recs, ops, ext = got
    bad = np.nonzero((recs != exp[0]).any(axis=1))[0]
    assert bad.size == 0, (what, "records of pairs", bad[:8].tolist(), "got", recs[bad[:4]].tolist(), "expected", exp[0][bad[:4]].tolist())
    for p, want in enumerate(exp[1]):
        assert ops[p, :len(want)].tolist() == want, (what, "ops of pair", p, ops[p, :len(want)].tolist()[:12], want[:12])
    bad = np.nonzero((ext != exp[2]).any(axis=1))[0]
    assert bad.size == 0, (what, "extension records of pairs", bad[:8].tolist(), ext[bad[:4]].tolist(), exp[2][bad[:4]].tolist())


@pytest.mark.parametrize("form", ["lin", "aff"])
def test_alignments_one_strip(form):
    R, F, band_width, Z = 33, 70, 40, 10
    sc, affine = _sc(form), _affine(form)
    rng = np.random.default_rng(17)
    reads, refs, drops = _one_strip_pairs(rng, R, F, sc, affine, Z, band_width)
    zrecords, T = ezr.extend(reads, refs, sc, Z, band_width, affine)
    Rp = extend_ref.trimmed_lengths(reads)
    assert drops
    _guards(zrecords, T, ebr.extend(reads, refs, sc, band_width, affine), Rp, rows=(7, 8) if form == "lin" else ())
    eng = _engine(R, F, sc, Z, band_width, align=1)
    for bonus in (-1, 0, 1000):
        exp = _align_expect(reads, refs, sc, affine, band_width, T, Rp, bonus, zrecords)
        if bonus == 1000:
            assert exp[0][3, 1] == R                    # the undropped pair ends in its read end
        _check_align(_run_align(eng, reads, refs, bonus, stride=40), exp, (form, bonus))
        d = eng.describe(0, 5)
        assert d["ran_extend_align"] == "band" and d["ran_extend_zdrop"] == Z and d["extend_zdrop_skipped_waves"] == 0, d
    eng.close()


@pytest.mark.parametrize("form", ["lin", "aff"])
@pytest.mark.parametrize("R", [513, 520])
def test_alignments_two_strips(R, form):
    F, band_width, Z = 600, 130, 10
    reads, refs, zrecords, T, count = _two_strip_case(R, F, form, band_width)
    reads, refs = reads.copy(), refs.copy()
    sc, affine = _sc(form), _affine(form)
    Rp = extend_ref.trimmed_lengths(reads)
    eng = _engine(R, F, sc, Z, band_width, align=1)
    for bonus in (-1, 0, 1000):
        exp = _align_expect(reads, refs, sc, affine, band_width, T, Rp, bonus, zrecords)
        _check_align(_run_align(eng, reads, refs, bonus, stride=64), exp, (R, form, bonus))
        d = eng.describe(0, len(reads))
        assert d["ran_extend_align"] == "band" and d["extend_zdrop_skipped_waves"] == count, (d["ran_extend_align"], d["extend_zdrop_skipped_waves"], count)
    eng.close()


# ---- 5. refusals with their texts, key changes on a live engine, the host entry ----
def test_refusals():
    R, F = 33, 70
    rng = np.random.default_rng(5)
    pairs = [_plant(BASES[rng.integers(0, 4, R)], F, a) for a in (5, 9, 14, 20)]
    reads, refs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    sc = _sc("sym")
    eng = _engine(R, F, sc, 10)
    exp, _ = ezr.extend(reads, refs, sc, 10)
    _check(_run(eng, reads, refs), exp, "before the refusals")

    def refused(call, text):
        with pytest.raises(hipkernel.HipKernelError) as err:
            call()
        assert str(err.value) == text, str(err.value)

    eng.set_score_width(16)
    for call in (lambda: eng.score_extend_device(0, d_reads, d_refs), lambda: eng.score_extend_host(0, reads, refs)):
        refused(call, TEXT_NO_INT16)
        assert eng.describe(0, 4)["ran_extend"] == "none" and eng.describe(0, 4)["ran_extend_zdrop"] == 0
    eng.set_score_width(0)
    # alignments without a band, and under a band without the two keys
    for band_width, band, align in ((0, 0, 0), (0, 1, 1), (40, 1, 0), (40, 0, 1)):
        eng.set_band_width(band_width)
        eng.set_extend_band(band)
        eng.set_extend_band_align(align)
        for call in (lambda: eng.align_extend_device(0, d_reads, d_refs), lambda: eng.align_extend_host(0, reads, refs)):
            refused(call, TEXT_ALIGN)
            assert eng.describe(0, 4)["ran_extend_align"] == "none"
    eng.set_band_width(0)
    eng.set_extend_band(0)
    eng.set_extend_band_align(0)
    for Z in (-1, (1 << 30) + 1):
        refused(lambda: eng.set_extend_zdrop(Z), TEXT_KEY)
        assert eng.describe(0, 4)["extend_zdrop"] == 10
    eng.set_extend_zdrop(1 << 30)
    assert eng.describe(0, 4)["extend_zdrop"] == 1 << 30
    eng.set_extend_zdrop(10)
    # the mode bit and the policy keep their texts, and come first
    with pytest.raises(hipkernel.HipKernelError, match="opt & 0xF == 0 only"):
        eng.score_extend_device(1, d_reads, d_refs)
    eng.set_traceback_policy(1)
    with pytest.raises(hipkernel.HipKernelError, match="traceback_policy = 1"):
        eng.score_extend_device(0, d_reads, d_refs)
    eng.set_traceback_policy(0)
    _check(_run(eng, reads, refs), exp, "after the refusals")
    eng.close()


def test_key_changes_on_a_live_engine():
    R, F, band_width = 520, 600, 130
    sc, affine = _sc("aff"), True
    rng = np.random.default_rng(11)
    pairs = [_plant(BASES[rng.integers(0, 4, R)], F, a) for a in (60, 300, 505, 100)] + [_whole(rng, R, F)]
    reads, refs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    live = hipkernel.Engine(R, F, sc)
    live.set_extend_wide(1)
    live.set_score_width(32)
    seen = []
    for Z, band in ((0, 0), (10, 0), (10, band_width), (0, band_width), (0, 0), (30, 0), (30, band_width)):
        for eng in (live, None):
            if eng is None:
                eng = fresh = hipkernel.Engine(R, F, sc)
                eng.set_extend_wide(1)
                eng.set_score_width(32)
            eng.set_band_width(band)
            eng.set_extend_band(1 if band else 0)
            eng.set_extend_zdrop(Z)
        exp, T = ezr.extend(reads, refs, sc, Z, band, affine, chunk=5) if Z else (_free(reads, refs, sc, band, affine), None)
        got, again = _run(live, reads, refs), _run(fresh, reads, refs)
        _check(got, exp, ("live", Z, band))
        _check(again, exp, ("fresh", Z, band))
        a, b = live.describe(0, 5), fresh.describe(0, 5)
        for key in ("ran_extend", "extend_zdrop", "ran_extend_zdrop", "extend_zdrop_skipped_waves"):
            assert a[key] == b[key], (key, Z, band, a[key], b[key])
        assert a["ran_extend_zdrop"] == Z
        fresh.close()
        seen.append(exp)
    assert (seen[0] != seen[1]).any() and (seen[1] != seen[5]).any(), "Z changes no record"
    live.close()


def test_host_entry():
    R, F, n, Z = 520, 600, 21, 10
    sc = _sc("lin")
    rng = np.random.default_rng(23)
    pairs = [_plant(BASES[rng.integers(0, 4, R)], F, int(rng.integers(5, 500))) if k % 5 else _whole(rng, R, F) for k in range(n)]
    reads, refs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    exp, T = ezr.extend(reads, refs, sc, Z, chunk=7)
    _guards(exp, T, extend_ref.extend(reads, refs, sc, chunk=7), extend_ref.trimmed_lengths(reads))
    eng = _engine(R, F, sc, Z)
    dev = _run(eng, reads, refs)
    _check(dev, exp, "device")
    for threads in (1, 3):
        _check(_host(eng, reads, refs, threads), exp, ("host", threads))
        assert eng.describe(0, n)["ran_extend"] == "wide" and eng.describe(0, n)["ran_extend_zdrop"] == Z
    eng.close()
