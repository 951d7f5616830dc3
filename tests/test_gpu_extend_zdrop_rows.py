"""Extension Z-drop on the int16 register sweep (key extend_zdrop_rows; the ZDROP instances of score_extend_kernel and
align_extend_fill_kernel) on the GPU.  References, independent of the library: tests/extend_zdrop_ref.py with band_width = 0 for
the records and the drop rows T, tests/extend_align_ref.py on the reads cut at T for the alignments.  Integers, compared exactly:
all five fields of every record, and for alignments records, ops and extension records.

Inputs are planted: the reference follows the read down the diagonal except for runs of mismatching bases (_mismatch_pair), or for
14 bases of C against A (test_gpu_extend_zdrop._plant).  Under Z = 10 and the linear gaps -2 / -4 the fourth mismatching row in a
run drops (3 k > 10) and nothing else does, so a drop row can be named; under Z = 2 and the four-score affine form the first one
drops (a gap opens at -6 / -4, so no chance match beside the diagonal pays for one), so row 0 can drop; under the linear gaps a gap
of -2 and a chance match undo a single mismatch too often to name that row.  Where a gap is as cheap as a mismatch, or affine
under Z = 10, the gap path is the row's maximum and the penalty pays for it: the drop falls later, by an amount that depends
on the sequences -- there the pairs are chosen from the drop rows the reference shows over every start of the run, a lane's last
and first row where they occur.  Every case first asserts, on the reference alone, that some pair scores, that some record differs
from the one without the key, that the drop rows it names occur and that some pair runs to its end."""
import functools

import numpy as np
import pytest
import torch

import extend_align_ref as ear
import extend_ref
import extend_zdrop_ref as ezr
import instance_matrix as im
from test_gpu_extend import FORMS, FULL, _affine, _check, _host, _run, _scoring
from test_gpu_extend_align import _run as _run_align
from test_gpu_extend_zdrop import TEXT_ALIGN, TEXT_NO_INT16, _check_align, _guards, _plant, _plant_at, _whole
from versalignlib_amd import hipkernel

pytestmark = pytest.mark.gpu

BASES = np.frombuffer(b"ACGT", np.uint8)
NEVER = 1 << 29
TEXT_ROWS_ALIGN = ("extend_zdrop: the int32 route of unbanded extension alignments has no Z-drop form (extend_zdrop_rows = 1 runs Z-dropped "
                   "unbanded extension alignments on the int16 register sweep only; this call's shape, scoring or keys leave it)")
TEXT_ROWS_KEY = "extend_zdrop_rows must be 0 or 1"


def _sc(form):
    return _scoring(form, 2, -3)


def _engine(R, F, sc, Z, rows=1, geometry=None):
    eng = hipkernel.Engine(R, F, sc, group_lanes=geometry[0], rows_per_lane=geometry[1]) if geometry else hipkernel.Engine(R, F, sc)
    eng.set_extend_zdrop(Z)
    eng.set_extend_zdrop_rows(rows)
    return eng


def _mismatch_pair(rng, R, F, rows):
    """-> read, ref: the reference follows a random read down the diagonal, with another base at the rows listed"""
    read = BASES[rng.integers(0, 4, R)]
    ref = np.full(F, ord("T"), np.uint8)
    m = min(R, F)
    ref[:m] = read[:m]
    for r in rows:
        if r < m:
            ref[r] = BASES[(int(np.searchsorted(BASES, read[r])) + 1) % 4]
    return read, ref


def _hover_pair(R, F, T):
    """Z = 10, linear gaps -2 / -4: the running best at row 3, in lane 0; then periods of (mismatch, match, mismatch, match, match)
    -- 0 net, never above the best, at most 4 below it -- up to row T - 4, and from there A against C: row T is the fourth.  Chance
    matches beside the diagonal would lift a row's maximum (a gap of -2 and a match beat a mismatch), so the read is ACGT repeated,
    a mismatch is the next base of that order, and the reference ends with the read."""
    assert T % 5 == 2 and T >= 12 and R <= F
    read = BASES[np.arange(R) % 4]
    ref = np.zeros(F, np.uint8)
    ref[:R] = read
    for r in range(4, T - 3):
        if (r - 4) % 5 in (0, 2):
            ref[r] = BASES[(r + 1) % 4]
    read[T - 3:] = ord("A")
    ref[T - 3:R] = ord("C")
    return read, ref


def _ran(d, Z, geometry=None, align=False):
    name = "ran_extend_align" if align else "ran_extend"
    assert d[name] == "rows" and d["ran_extend_zdrop"] == Z and d["extend_zdrop"] == Z and d["extend_zdrop_rows"] == 1, (d[name], d["ran_extend_zdrop"], d["extend_zdrop_rows"])
    assert d["extend_zdrop_skipped_waves"] == 0, d["extend_zdrop_skipped_waves"]
    if geometry:
        assert d[name + "_geometry"] == "%dx%d" % geometry, (geometry, d[name + "_geometry"])


def _align_expect(reads, refs, sc, affine, T, Rp, bonuses, zrecords):
    """-> one expectation per bonus: the alignment of the pair cut to its first T rows, from its best cell where the pair dropped"""
    cut = ezr.cut_reads(reads, T)
    res = ear.align(cut, refs, sc, affine, end_bonus=(-1,) + tuple(bonuses), chunk=16)
    best, dropped, out = res[0], T < Rp, []
    for chosen in res[1:]:
        recs = np.where(dropped[:, None], best[0], chosen[0])
        ops = [best[1][k] if dropped[k] else chosen[1][k] for k in range(len(reads))]
        for k in np.nonzero(dropped)[0]:                # the read end is never chosen where T < Rp
            assert recs[k, 1] <= T[k] and recs[k, 1] == zrecords[k, 1]
        out.append((recs, ops, zrecords, None))
    return out


def _stride(exps):
    return max([len(o) for e in exps for o in e[1]] + [1]) + 2


# ---- 1. every new instance: six geometries x four gap forms (scores), x {linear, affine} (alignments), forced ----
# (the references of these shapes are 7 to 135 columns long: under Z = 10 only the linear gaps -2 / -4 let a run of mismatches that
# short drop; the other forms run under Z = 2, where the first mismatch drops, or the first match behind two of them where a gap
# is as cheap as a mismatch)
INSTANCE_Z = {"lin": 10, "sym": 2, "affsym": 2, "aff": 2}


@functools.lru_cache(maxsize=None)
def _instance_case(G, K, shape, form):
    Z = INSTANCE_Z[form]
    R, F = im.shapes(G, K)[shape]
    n = im.batch(G)
    sc, affine = _sc(form), _affine(form)
    rng = np.random.default_rng(1000 * G + 10 * K + shape)
    m = min(R, F)
    pairs = []
    for k in range(n):
        if k % 4 == 3:                                  # never drops: the read ends with the reference (the gap down the last column
            pairs.append(_whole(rng, R, F))             # opens at a price Z = 2 does not cover)
            pairs[-1][0][m:] = ord("N")
        elif k % 4 == 1:                                # a run of mismatches to the end, from inside any lane the reference reaches
            pairs.append(_mismatch_pair(rng, R, F, range(int(rng.integers(1, m)), R)))
        elif k % 4 == 2:                                # two mismatches, then the homology again
            a = int(rng.integers(1, max(2, m - 3)))
            pairs.append(_mismatch_pair(rng, R, F, (a, a + 1)))
        else:
            pairs.append(_plant(BASES[rng.integers(0, 4, R)], F, int(rng.integers(1, max(2, m - 4)))))
    reads, refs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    reads[2, R - K - 2:] = ord("N")                     # the halves of a register differ in Rp and Fp
    refs[5, F - 2:] = 0
    exp, T = ezr.extend(reads, refs, sc, Z, 0, affine, chunk=16)
    free = extend_ref.extend(reads, refs, sc, affine=affine, chunk=16)
    Rp = extend_ref.trimmed_lengths(reads)
    _guards(exp, T, free, Rp)
    for a in (reads, refs, exp, T):
        a.setflags(write=False)
    return reads, refs, exp, T, Rp


@pytest.mark.parametrize("shape", range(4))
@pytest.mark.parametrize("G,K", FULL)
def test_every_score_instance(G, K, shape):
    R, F = im.shapes(G, K)[shape]
    for form in FORMS:
        reads, refs, exp, T, Rp = _instance_case(G, K, shape, form)
        eng = _engine(R, F, _sc(form), INSTANCE_Z[form], geometry=(G, K))
        got = _run(eng, reads.copy(), refs.copy())
        d = eng.describe(0, len(reads))
        eng.close()
        _check(got, exp, (G, K, R, F, form))
        _ran(d, INSTANCE_Z[form], (G, K))


@pytest.mark.parametrize("shape", range(4))
@pytest.mark.parametrize("G,K", FULL)
def test_every_fill_instance(G, K, shape):
    R, F = im.shapes(G, K)[shape]
    for form in ("lin", "aff"):
        reads, refs, zrecords, T, Rp = _instance_case(G, K, shape, form)
        reads, refs = reads.copy(), refs.copy()
        bonuses = (-1, ear.INT32_MAX)
        exps = _align_expect(reads, refs, _sc(form), _affine(form), T, Rp, bonuses, zrecords)
        assert any(e is not None for e in ear.align(ezr.cut_reads(reads, T), refs, _sc(form), _affine(form), chunk=16)[3])
        eng = _engine(R, F, _sc(form), INSTANCE_Z[form], geometry=(G, K))
        for bonus, exp in zip(bonuses, exps):
            _check_align(_run_align(eng, reads, refs, bonus, stride=_stride(exps)), exp, (G, K, R, F, form, bonus))
            _ran(eng.describe(0, len(reads)), INSTANCE_Z[form], (G, K), align=True)
        eng.close()


# ---- 2. lane, group and register edges on 8 x 8 (33 x 70) and 16 x 10 (150 x 160) ----
EDGES = [((8, 8), 33, 70), ((16, 10), 150, 160)]


def _from_table(rng, R, F, sc, affine, Z, K):
    """planted pairs by drop row, over every start of the run of C, on the reference: -> {T: (read, ref)}, a lane's last row and a
    lane's first row first where they occur"""
    base = BASES[rng.integers(0, 4, R)]
    table = [_plant(base, F, a) for a in range(1, R - 1)]
    _, rows = ezr.extend(np.stack([p[0] for p in table]), np.stack([p[1] for p in table]), sc, Z, 0, affine, chunk=32)
    first = {}
    for k, T in enumerate(rows.tolist()):
        if T < R:
            first.setdefault(T, table[k])
    order = [T for T in first if T % K == K - 1][:1] + [T for T in first if T % K == 0][:1]
    order += [T for T in sorted(first) if T not in order]
    return first, order


@functools.lru_cache(maxsize=None)
def _edge_case(geometry, R, F, form, Z):
    """-> reads, refs, records, T, Rp of one full wave plus one pair.  Pairs 2 k and 2 k + 1 share a register."""
    G, K = geometry
    sc, affine = _sc(form), _affine(form)
    rng = np.random.default_rng(R * F + Z)
    n = 2 * (64 // G) + 1
    last_lane_T = {33: 32, 150: 147}[R]                 # = 2 mod 5, in the last lane that holds a row of the read
    assert last_lane_T // K == (R - 1) // K and last_lane_T // K > 1
    literal = (form == "lin" and Z == 10) or (form == "aff" and Z == 2)
    if form == "lin" and Z == 10:
        named = (K - 1, K, last_lane_T, R - 1)
        at = lambda T: _plant_at(rng, R, F, sc, affine, Z, 0, T, tries=8)
        drops = [at(K - 1), at(K), _hover_pair(R, F, last_lane_T), at(R - 1)]
    elif literal:                                       # Z = 2: the first mismatching row drops, row 0 included
        named = (0, K - 1, K, last_lane_T, R - 1)
        drops = [_mismatch_pair(rng, R, F, range(T, R)) for T in (K - 1, K, last_lane_T, R - 1, 0)]
    else:                                               # rows as they fall (see the module's text)
        first, order = _from_table(rng, R, F, sc, affine, Z, K)
        assert len(order) >= 3, (form, Z, order)
        named = tuple(order[:4])
        drops = [first[T] for T in order[:4]]
    short = list(_whole(rng, R, F))                     # an undropped pair with an Rp and an Fp of its own
    short[0][K + 3:] = ord("N")
    short[1][F - 5:] = 0
    rp0 = (np.full(R, ord("N"), np.uint8), _whole(rng, R, F)[1])
    fp0 = (BASES[rng.integers(0, 4, R)], np.zeros(F, np.uint8))
    never = (np.full(R, ord("A"), np.uint8), np.full(F, ord("C"), np.uint8))           # M = 0 throughout
    #        a dropped and an undropped half   ... and the reverse       the group's last lane / Rp - 1             (Z = 2: row 0)
    pairs = [drops[0], _whole(rng, R, F), tuple(short), drops[1], drops[2], drops[min(3, len(drops) - 1)], rp0, fp0] + (drops[4:] or [never]) + [never]
    while len(pairs) < n:
        k = len(pairs)
        pairs.append(_whole(rng, R, F) if k % 3 == 0 else _plant(BASES[rng.integers(0, 4, R)], F, int(rng.integers(1, R - 16))))
    reads, refs = np.stack([p[0] for p in pairs[:n]]), np.stack([p[1] for p in pairs[:n]])
    exp, T = ezr.extend(reads, refs, sc, Z, 0, affine, chunk=16)
    free = extend_ref.extend(reads, refs, sc, affine=affine, chunk=16)
    Rp, Fp = extend_ref.trimmed_lengths(reads), extend_ref.trimmed_lengths(refs)
    _guards(exp, T, free, Rp, rows=named)
    # the halves of register 0 and of register 1: dropped / undropped and the reverse, with different Rp and Fp in register 1
    assert T[0] < Rp[0] and T[1] == Rp[1] and T[2] == Rp[2] and T[3] < Rp[3] and Rp[2] == K + 3 and Rp[3] == R and Fp[2] == F - 5 and Fp[3] > Fp[2]
    assert Rp[6] == 0 and exp[6].tolist() == [0, 0, 0, 0, 0] and Fp[7] == 0 and exp[7, :3].tolist() == [0, 0, 0]
    if literal:
        assert T[0] == K - 1 and T[3] == K and T[4] == last_lane_T and T[5] == R - 1, T[:6].tolist()
        if Z == 10:
            assert 0 < exp[4, 1] <= K, exp[4].tolist()          # ... with the running best in lane 0
        else:
            assert T[8] == 0 and exp[8].tolist() == [0, 0, 0, ezr.UNREACHED, 0]
    for a in (reads, refs, exp, T):
        a.setflags(write=False)
    return reads, refs, exp, T, Rp


EDGE_RUNS = [(form, 10) for form in FORMS] + [("aff", 2)]


@pytest.mark.parametrize("form,Z", EDGE_RUNS)
@pytest.mark.parametrize("geometry,R,F", EDGES)
def test_edges(geometry, R, F, form, Z):
    reads, refs, exp, T, Rp = _edge_case(geometry, R, F, form, Z)
    eng = _engine(R, F, _sc(form), Z, geometry=geometry)
    for n in (len(reads), 1, 5, len(reads) - 1):        # a full wave plus one pair, one pair, an odd last register, a full wave
        _check(_run(eng, reads[:n].copy(), refs[:n].copy()), exp[:n], (geometry, form, Z, n))
        _ran(eng.describe(0, n), Z, geometry)
    eng.close()


# ---- 3. identities ----
@pytest.mark.parametrize("form", list(FORMS))
def test_identities(form):
    geometry, R, F = EDGES[1]
    reads, refs, exp, T, Rp = _edge_case(geometry, R, F, form, 10)
    reads, refs = reads.copy(), refs.copy()
    sc, affine = _sc(form), _affine(form)
    free = extend_ref.extend(reads, refs, sc, affine=affine, chunk=16)
    off = hipkernel.Engine(R, F, sc)                    # both keys off; the plan is the engine's own (re-planned onto a full geometry)
    plain = _run(off, reads, refs)
    _check(plain, free, (form, "both keys off"))
    assert off.describe(0, len(reads))["ran_extend"] == "rows"
    eng = _engine(R, F, sc, NEVER)
    never = _run(eng, reads, refs)
    _ran(eng.describe(0, len(reads)), NEVER)
    assert np.array_equal(never, plain), (form, "Z = 2^29 under the key is the record with both keys off, bit for bit")
    eng.set_extend_zdrop(0)                             # the key on with Z = 0 is the key off
    zero = _run(eng, reads, refs)
    d = eng.describe(0, len(reads))
    assert np.array_equal(zero, plain) and d["ran_extend"] == "rows" and d["ran_extend_zdrop"] == 0 and d["extend_zdrop_rows"] == 1
    eng.set_extend_zdrop(10)
    on = _run(eng, reads, refs)
    _ran(eng.describe(0, len(reads)), 10)
    eng.set_extend_zdrop_rows(0)                        # the same call on today's route
    wide = _run(eng, reads, refs)
    d = eng.describe(0, len(reads))
    assert d["ran_extend"] == "wide" and d["ran_extend_zdrop"] == 10 and d["extend_zdrop_rows"] == 0
    _check(on, exp, (form, "rows"))
    assert np.array_equal(on, wide), (form, "the register sweep and the strip sweep give the same records")
    off.close()
    eng.close()


# ---- 4. alignments: three end bonuses, records, ops and extension records ----
@pytest.mark.parametrize("form,Z", [("lin", 10), ("aff", 10), ("aff", 2)])
@pytest.mark.parametrize("geometry,R,F", EDGES)
def test_alignments(geometry, R, F, form, Z):
    reads, refs, zrecords, T, Rp = _edge_case(geometry, R, F, form, Z)
    reads, refs = reads.copy(), refs.copy()
    sc, affine = _sc(form), _affine(form)
    bonuses = (-1, 0, 1000)
    exps = _align_expect(reads, refs, sc, affine, T, Rp, bonuses, zrecords)
    assert exps[2][0][1, 1] == R and (exps[2][0][T < Rp, 1] < Rp[T < Rp]).all()          # 1000 picks the read end of the undropped pairs only
    assert (exps[0][0][:, 5] > 0).any()
    eng = _engine(R, F, sc, Z, geometry=geometry)
    for bonus, exp in zip(bonuses, exps):
        for n in (len(reads), 5):
            got = _run_align(eng, reads[:n].copy(), refs[:n].copy(), bonus, stride=_stride(exps))
            _check_align(got, (exp[0][:n], exp[1][:n], exp[2][:n], None), (geometry, form, Z, bonus, n))
            _ran(eng.describe(0, n), Z, geometry, align=True)
    # without the extension records, and the unforced plan
    got = _run_align(eng, reads, refs, 0, stride=_stride(exps), with_extend=False)
    assert got[2] is None and np.array_equal(got[0], exps[1][0])
    eng.close()
    eng = _engine(R, F, sc, Z)
    _check_align(_run_align(eng, reads, refs, 0, stride=_stride(exps)), exps[1], (form, Z, "the engine's own plan"))
    _ran(eng.describe(0, len(reads)), Z, align=True)
    eng.close()


# ---- 5. routes and refusals ----
def _refused(call, text):
    with pytest.raises(hipkernel.HipKernelError) as err:
        call()
    assert str(err.value) == text, str(err.value)


def test_routes_and_refusals():
    geometry, R, F = EDGES[0]
    reads, refs, exp, T, Rp = _edge_case(geometry, R, F, "sym", 10)
    reads, refs = reads.copy(), refs.copy()
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    sc, n = _sc("sym"), len(reads)
    eng = _engine(R, F, sc, 10)
    # score_width = 16 runs with the key on and keeps its text with the key off
    eng.set_score_width(16)
    _check(_run(eng, reads, refs), exp, "score_width = 16 under the key")
    _ran(eng.describe(0, n), 10)
    eng.set_extend_zdrop_rows(0)
    for call in (lambda: eng.score_extend_device(0, d_reads, d_refs), lambda: eng.score_extend_host(0, reads, refs)):
        _refused(call, TEXT_NO_INT16)
        assert eng.describe(0, n)["ran_extend"] == "none" and eng.describe(0, n)["ran_extend_zdrop"] == 0
    # alignments with the key off keep their text
    eng.set_score_width(0)
    for call in (lambda: eng.align_extend_device(0, d_reads, d_refs), lambda: eng.align_extend_host(0, reads, refs)):
        _refused(call, TEXT_ALIGN)
        assert eng.describe(0, n)["ran_extend_align"] == "none"
    eng.set_extend_zdrop_rows(1)
    # score_width = 32 still runs "wide"; alignments there are on the int32 route: the new text
    eng.set_score_width(32)
    _check(_run(eng, reads, refs), exp, "score_width = 32")
    d = eng.describe(0, n)
    assert d["ran_extend"] == "wide" and d["ran_extend_zdrop"] == 10 and d["extend_zdrop_rows"] == 1
    for call in (lambda: eng.align_extend_device(0, d_reads, d_refs), lambda: eng.align_extend_host(0, reads, refs)):
        _refused(call, TEXT_ROWS_ALIGN)
        assert eng.describe(0, n)["ran_extend_align"] == "none"
    eng.set_score_width(0)
    # a band answers as today: scores refused without extend_band, "band" with it; alignments keep the older text off the banded route
    eng.set_band_width(40)
    with pytest.raises(hipkernel.HipKernelError, match="not built for band_width > 0"):
        eng.score_extend_device(0, d_reads, d_refs)
    _refused(lambda: eng.align_extend_device(0, d_reads, d_refs), TEXT_ALIGN)
    eng.set_extend_band(1)
    banded, _ = ezr.extend(reads, refs, sc, 10, 40)
    _check(_run(eng, reads, refs), banded, "under a band")
    assert eng.describe(0, n)["ran_extend"] == "band"
    _refused(lambda: eng.align_extend_device(0, d_reads, d_refs), TEXT_ALIGN)
    eng.set_extend_band_align(1)
    eng.align_extend_device(0, d_reads, d_refs)
    assert eng.describe(0, n)["ran_extend_align"] == "band"
    eng.set_band_width(0)
    eng.set_extend_band(0)
    eng.set_extend_band_align(0)
    # the key's own range, the mode bit and the policy
    for on in (-1, 2):
        _refused(lambda: eng.set_extend_zdrop_rows(on), TEXT_ROWS_KEY)
        assert eng.describe(0, n)["extend_zdrop_rows"] == 1
    with pytest.raises(hipkernel.HipKernelError, match="opt & 0xF == 0 only"):
        eng.score_extend_device(1, d_reads, d_refs)
    eng.set_traceback_policy(1)
    for call in (lambda: eng.score_extend_device(0, d_reads, d_refs), lambda: eng.align_extend_device(0, d_reads, d_refs)):
        with pytest.raises(hipkernel.HipKernelError, match="traceback_policy = 1"):
            call()
    eng.set_traceback_policy(0)
    _check(_run(eng, reads, refs), exp, "after the refusals")
    _ran(eng.describe(0, n), 10)
    eng.close()
    # cells that leave int16 run "wide" (score_width = 0), as a read of 1,500 rows does
    wide_sc = hipkernel.Scoring.make(970, -3, -2, -4)
    eng = _engine(R, F, wide_sc, 10)
    _check(_run(eng, reads, refs), ezr.extend(reads, refs, wide_sc, 10)[0], "cells outside int16")
    assert eng.describe(0, n)["ran_extend"] == "wide"
    _refused(lambda: eng.align_extend_device(0, d_reads, d_refs), TEXT_ROWS_ALIGN)
    eng.close()
    R2, F2 = 1500, 64
    rng = np.random.default_rng(3)
    pairs = [_plant(BASES[rng.integers(0, 4, R2)], F2, a) for a in (5, 30)] + [_whole(rng, R2, F2)]
    long_reads, long_refs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    eng = _engine(R2, F2, _sc("lin"), 10)
    _check(_run(eng, long_reads, long_refs), ezr.extend(long_reads, long_refs, _sc("lin"), 10)[0], "a read of 1,500 rows")
    assert eng.describe(0, 3)["ran_extend"] == "wide"
    _refused(lambda: eng.align_extend_device(0, torch.from_numpy(long_reads).cuda(), torch.from_numpy(long_refs).cuda()), TEXT_ROWS_ALIGN)
    eng.close()


# ---- 6. key changes on one live engine against fresh ones, and the host entries ----
def test_key_changes_on_a_live_engine():
    geometry, R, F = EDGES[1]
    form = "aff"
    sc, affine = _sc(form), True
    reads, refs, _, _, Rp = _edge_case(geometry, R, F, form, 2)
    reads, refs = reads.copy(), refs.copy()
    free = extend_ref.extend(reads, refs, sc, affine=affine, chunk=16)
    live = hipkernel.Engine(R, F, sc)
    seen = []
    for Z, rows in ((0, 0), (2, 1), (2, 0), (10, 1), (0, 1), (2, 1), (NEVER, 1), (10, 0)):
        fresh = hipkernel.Engine(R, F, sc)
        for eng in (live, fresh):
            eng.set_extend_zdrop(Z)
            eng.set_extend_zdrop_rows(rows)
        exp, T = ezr.extend(reads, refs, sc, Z, 0, affine, chunk=16) if Z else (free, None)
        _check(_run(live, reads, refs), exp, ("live", Z, rows))
        _check(_run(fresh, reads, refs), exp, ("fresh", Z, rows))
        a, b = live.describe(0, len(reads)), fresh.describe(0, len(reads))
        for key in ("ran_extend", "ran_extend_geometry", "extend_zdrop", "ran_extend_zdrop", "extend_zdrop_skipped_waves", "extend_zdrop_rows"):
            assert a[key] == b[key], (key, Z, rows, a[key], b[key])
        assert a["ran_extend"] == ("wide" if Z and not rows else "rows") and a["ran_extend_zdrop"] == Z
        if Z and rows:                                  # ... and the alignments of the same engine, between the score calls
            exps = _align_expect(reads, refs, sc, affine, T, Rp, (0,), exp)
            for eng in (live, fresh):
                _check_align(_run_align(eng, reads, refs, 0, stride=_stride(exps)), exps[0], ("alignments", Z))
                _ran(eng.describe(0, len(reads)), Z, align=True)
        fresh.close()
        seen.append(exp)
    assert (seen[0] != seen[1]).any() and (seen[1] != seen[3]).any() and np.array_equal(seen[1], seen[2]), "Z changes no record"
    live.close()


def test_host_entries():
    R, F, n, Z = 150, 160, 41, 10
    sc, affine = _sc("lin"), False
    rng = np.random.default_rng(29)
    pairs = [_plant(BASES[rng.integers(0, 4, R)], F, int(rng.integers(5, 130))) if k % 5 else _whole(rng, R, F) for k in range(n)]
    reads, refs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    exp, T = ezr.extend(reads, refs, sc, Z, chunk=16)
    Rp = extend_ref.trimmed_lengths(reads)
    _guards(exp, T, extend_ref.extend(reads, refs, sc, chunk=16), Rp)
    eng = _engine(R, F, sc, Z)
    _check(_run(eng, reads, refs), exp, "device")
    for threads in (1, 3):
        _check(_host(eng, reads, refs, threads), exp, ("host", threads))
        _ran(eng.describe(0, n), Z)
    want = _align_expect(reads, refs, sc, affine, T, Rp, (6,), exp)[0]
    dev = _run_align(eng, reads, refs, 6, stride=_stride([want]))
    _check_align(dev, want, "alignments, device")
    for with_extend in (True, False):
        recs, ops, offsets, ext = eng.align_extend_host(0, reads, refs, end_bonus=6, with_extend=with_extend, threads=2)
        assert (np.stack([recs[k] for k in hipkernel.aln_dtype().names], axis=1).astype(np.int64) == want[0]).all(), with_extend
        assert offsets[0] == 0 and (np.diff(offsets) == want[0][:, 5]).all() and len(ops) == offsets[n]
        for p in range(n):
            assert ops[offsets[p]:offsets[p + 1]].tolist() == want[1][p], p
        if with_extend:
            assert (np.stack([ext[k] for k in hipkernel.extend_dtype().names], axis=1).astype(np.int64) == exp).all()
        _ran(eng.describe(0, n), Z, align=True)
    eng.close()
