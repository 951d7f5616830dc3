"""Placed Smith-Waterman scores on the GPU (valign_hip_score_placed_device / _host): score and end cell of every pair from the
score sweep, against tests/placed_ref.py (numpy, int64 cells, independent of the library) unless a test says otherwise.

The rule that picks the path (placed_choice, cell_rules.h) is restated here in three lines (`_predict`) so that
describe()["ran_placed"] is checked against a prediction, not against itself."""
import functools

import numpy as np
import pytest
import torch

import placed_ref
from conftest import debug_switches
from versalignlib_amd import hipkernel, synth

pytestmark = pytest.mark.gpu

FULL = [(8, 8), (16, 10), (32, 10), (64, 8), (64, 16), (64, 32)]
# linear symmetric, linear gap_read != gap_ref, affine symmetric, affine with four scores
FORMS = {"sym": (-3, -3), "lin": (-2, -4), "affsym": (-3, -3, -5, -1, -5, -1), "aff": (-3, -3, -6, -2, -4, -1)}


def _scoring(form, match=2, mismatch=-1):
    return hipkernel.Scoring.make(match, mismatch, *FORMS[form])


def _predict(R, F, match, K, forced):
    if not forced and R > 1024:
        return "strip"
    bits = 2 if K <= 4 else (3 if K <= 8 else 4)
    return "key" if K <= 16 and ((min(R, F) * max(match, 0) + 1) << bits) <= 32000 else "rows"


def _pairs(n, R, F, seed, **kw):
    args = dict(sub_rate=0.1, indel_rate=0.02, n_run_frac=0.1, short_frac=0.1, lowercase_frac=0.05, junk_frac=0.04)
    args.update(kw)
    return synth.make_pairs(n, R, F, seed=seed, **args)


def _run(eng, reads, refs, opt=0):
    out = eng.score_placed_device(opt, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def _check(got, exp, what):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (what, "pairs", bad[:8].tolist(), "got", got[bad[:4]].tolist(), "expected", exp[bad[:4]].tolist())


@functools.lru_cache(maxsize=None)
def _case(R, F, form, seed, match=2):
    reads, refs = _pairs(64, R, F, seed)
    sc = _scoring(form, match)
    exp = placed_ref.placed(reads, refs, sc, affine=len(FORMS[form]) > 2)
    exp.setflags(write=False)
    return reads, refs, exp


# ---- 1. geometries ----
@pytest.mark.parametrize("R,F", [(12, 20), (33, 70), (40, 9), (64, 128), (150, 500), (300, 64)])
def test_register_geometries(R, F):
    for form in FORMS:
        reads, refs, exp = _case(R, F, form, 11 * R + F)
        sc = _scoring(form)
        for G, K in [(0, 0)] + [g for g in FULL if g[0] * g[1] >= R]:
            eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
            got = _run(eng, reads, refs)
            d = eng.describe(0, 64)
            eng.close()
            _check(got, exp, (R, F, form, G, K))
            k_ran = K or d["rows_per_lane"]
            assert d["ran_placed"] == _predict(R, F, 2, k_ran, bool(G)), (R, F, form, G, K, d["ran_placed"])
            if G:               # a full geometry carries every placed kernel: the call ran on the forced one
                assert d["ran_placed_geometry"] == "%dx%d" % (G, K), (R, F, form, G, K, d["ran_placed_geometry"])


def test_rows_form_on_64x24_and_forced_8x4_symmetric_there_asymmetric_replanned():
    """64 x 24 carries the rows track with all four forms.  8 x 4 carries the key track with the symmetric forms only: forced there,
    the calls with gap_read != gap_ref and with four affine scores are moved to a full geometry, and say so."""
    for form in FORMS:
        reads, refs, exp = _case(1000, 200, form, 5)
        eng = hipkernel.Engine(1000, 200, _scoring(form), group_lanes=64, rows_per_lane=24)
        got = _run(eng, reads, refs)
        d = eng.describe(0, 64)
        assert d["ran_placed"] == "rows" and d["ran_placed_geometry"] == "64x24", (form, d["ran_placed"], d["ran_placed_geometry"])
        eng.close()
        _check(got, exp, ("64x24", form))
        reads, refs, exp = _case(12, 20, form, 6)
        eng = hipkernel.Engine(12, 20, _scoring(form), group_lanes=8, rows_per_lane=4)
        got = _run(eng, reads, refs)
        d = eng.describe(0, 64)
        assert d["ran_placed"] == "key"
        if form in ("sym", "affsym"):
            assert d["ran_placed_geometry"] == "8x4", (form, d["ran_placed_geometry"])
        else:
            assert d["ran_placed_geometry"] != "8x4" and tuple(int(v) for v in d["ran_placed_geometry"].split("x")) in FULL, (form, d["ran_placed_geometry"])
        eng.close()
        _check(got, exp, ("forced 8x4, ran on " + d["ran_placed_geometry"], form))


# ---- 2. ties, built deliberately (forced 16 x 10 at 150 x 200: lane = (row + 10) // 10) ----
TR, TF = 150, 200


def _blank(n):
    return np.full((n, TR), ord("N"), np.uint8), np.full((n, TF), ord("N"), np.uint8)


def _motifs(rng, m):
    a = rng.choice(np.frombuffer(b"ACGT", np.uint8), m)
    b = a.copy()
    b[::2] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), a[::2])]      # differs from a at every other base
    return a, b


def _tie_scoring(form, match):
    """a mismatch or a gap base costs more than two matches give: no path through a second motif beats a motif's own diagonal"""
    g = -(2 * match + 1)
    return hipkernel.Scoring.make(match, g, g, g) if form == "sym" else hipkernel.Scoring.make(match, g, g, g, g - 3, g, g - 1, g)


def _tie_batches():
    rng = np.random.default_rng(2024)
    out = {}
    # (a) one motif twice in the reference: same row, two columns -- the first column wins
    reads, refs = _blank(16)
    for p in range(16):
        m = 10 + p % 5
        a, _ = _motifs(rng, m)
        r0, c0, c1 = 7 * p % 100, 3 + 5 * p % 60, 100 + 4 * p % 70
        reads[p, r0:r0 + m] = a
        refs[p, c0:c0 + m] = a
        refs[p, c1:c1 + m] = a
    out["ref_twice"] = (reads, refs, lambda p: (7 * p % 100 + 10 + p % 5, 3 + 5 * p % 60 + 10 + p % 5))
    # (b) two motifs of equal score in the read, the LATER one matching EARLIER in the reference: the earlier row wins.
    #     different lanes: motifs of 12 rows ending in rows 11 + s and 51 + s; same lane: 3 rows ending in rows 22 and 28
    for name, m, first, second in (("rows_in_two_lanes", 12, 0, 40), ("rows_in_one_lane", 3, 20, 26)):
        reads, refs = _blank(16)
        shifts = [p % 2 if name == "rows_in_two_lanes" else 0 for p in range(16)]
        cols = [120 + 3 * p for p in range(16)]
        for p in range(16):
            a, b = _motifs(rng, m)
            reads[p, first + shifts[p]:first + shifts[p] + m] = a
            reads[p, second + shifts[p]:second + shifts[p] + m] = b
            refs[p, 5 + p:5 + p + m] = b
            refs[p, cols[p]:cols[p] + m] = a
        out[name] = (reads, refs, lambda p, m=m, first=first, shifts=shifts, cols=cols: (first + shifts[p] + m, cols[p] + m))
    # (c) the maximum in row 0, in the last row, in column 0, in the last column: one matching base, everything else N
    reads, refs = _blank(16)
    spots = [(0, 17), (TR - 1, 5), (9, 0), (11, TF - 1), (0, 0), (TR - 1, TF - 1), (0, TF - 1), (TR - 1, 0)]
    for p in range(16):
        r, c = spots[p % 8]
        reads[p, r] = refs[p, c] = b"ACGT"[p % 4]
    out["borders"] = (reads, refs, lambda p: (spots[p % 8][0] + 1, spots[p % 8][1] + 1))
    # (d) half the pairs all-N
    reads, refs = _pairs(16, TR, TF, 77)
    reads[::2] = ord("N")
    out["half_empty"] = (reads, refs, None)
    return out


@pytest.mark.parametrize("form", ["sym", "aff"])
@pytest.mark.parametrize("match,track", [(2, "key"), (100, "rows")])
def test_ties(match, track, form):
    sc = _tie_scoring(form, match)
    eng = hipkernel.Engine(TR, TF, sc, group_lanes=16, rows_per_lane=10)
    for name, (reads, refs, where) in _tie_batches().items():
        assert not np.array_equal(reads[0], reads[1]) or not np.array_equal(refs[0], refs[1]), name       # pair A and pair B of a lane group differ
        got = _run(eng, reads, refs)
        assert eng.describe(0, 16)["ran_placed"] == track
        exp = placed_ref.placed(reads, refs, sc, affine=form == "aff")
        _check(got, exp, (name, track, form))
        if where:           # ... and the construction says where, independently of any fill
            for p in range(len(reads)):
                assert tuple(got[p, 1:]) == where(p), (name, p, got[p].tolist(), where(p))
        if name == "half_empty":
            assert not got[::2].any() and got[1::2, 0].all()
    eng.close()


# ---- 3. the key's range edge: last shape x match inside, first outside (cell_rules.h: (value + 1) << bits <= 32000) ----
@pytest.mark.parametrize("G,K,R,F,inside,outside", [(16, 10, 150, 500, 13, 14), (8, 4, 30, 100, 266, 267), (64, 16, 1000, 1100, 1, 2)])
def test_key_range_edge(G, K, R, F, inside, outside):
    reads, refs = synth.make_pairs(32, R, F, seed=R + K, sub_rate=0.0, n_run_frac=0.0, short_frac=0.0)      # perfect hits: the largest value occurs
    reads[16:], refs[16:] = _pairs(16, R, F, 3)
    for match, track in ((inside, "key"), (outside, "rows")):
        for form in ("sym", "affsym"):
            sc = _scoring(form, match)
            eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
            got = _run(eng, reads, refs)
            assert eng.describe(0, 32)["ran_placed"] == track, (match, form)
            eng.close()
            exp = placed_ref.placed(reads, refs, sc, affine=form == "affsym")
            assert exp[:16, 0].max() == R * match
            _check(got, exp, (G, K, match, form))


# ---- 4. ragged inputs and batch edges ----
def test_ragged_references_and_batch_edges():
    R, F = 150, 500
    rng = np.random.default_rng(9)
    reads, refs = _pairs(64, R, F, 41)
    for p in range(64):
        tail = int(F * rng.choice([0.0, 0.1, 0.5, 0.9]))
        if tail:
            refs[p, F - tail:] = 0
    refs[8:16, 50:] = 0             # a whole wave of 16 x 10 whose references are short: the trailing columns are skipped
    for form in ("sym", "aff"):
        sc = _scoring(form)
        exp = placed_ref.placed(reads, refs, sc, affine=form == "aff")
        eng = hipkernel.Engine(R, F, sc)
        ppw = eng.describe(0, 64)["pairs_per_wave"]
        for n in (64, 1, 7, ppw + 1):
            _check(_run(eng, reads[:n], refs[:n]), exp[:n], (form, n))
        eng.close()


# ---- 5. strips ----
@pytest.mark.parametrize("form", ["sym", "aff"])
@pytest.mark.parametrize("R", [1025, 1025 + 63])
def test_strips(R, form):
    F = 1300
    reads, refs = _pairs(6, R, F, R)
    # pair 2: two motifs of equal score, the first in strip 0 (rows 100-119), the second far below (rows 600-619) and matching
    # EARLIER in the reference: the earlier strip must win
    rng = np.random.default_rng(R)
    a, b = _motifs(rng, 20)
    reads[2] = ord("N")
    refs[2] = ord("N")
    reads[2, 100:120] = a
    reads[2, 600:620] = b
    refs[2, 50:70] = b
    refs[2, 700:720] = a
    sc = _scoring(form)
    eng = hipkernel.Engine(R, F, sc)
    got = _run(eng, reads, refs)
    assert eng.describe(0, 6)["ran_placed"] == "strip"
    eng.close()
    exp = placed_ref.placed(reads, refs, sc, affine=form == "aff")
    _check(got, exp, (R, form))
    assert tuple(got[2]) == (40, 120, 720), got[2]


def test_1024_rows_stay_on_the_register_sweep():
    reads, refs = _pairs(4, 1024, 300, 8)
    sc = _scoring("sym")
    eng = hipkernel.Engine(1024, 300, sc)
    got = _run(eng, reads, refs)
    assert eng.describe(0, 4)["ran_placed"] in ("key", "rows")
    eng.close()
    _check(got, placed_ref.placed(reads, refs, sc), "1024 x 300")


# ---- 6. cross-check with the existing paths on the same engine ----
@pytest.mark.parametrize("R,F", [(150, 500), (1025, 1300)])
@pytest.mark.parametrize("form", ["sym", "affsym"])
def test_agrees_with_scores_and_cigar_records(R, F, form):
    reads, refs = _pairs(256, R, F, R + 1)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    eng = hipkernel.Engine(R, F, _scoring(form))
    placed = eng.score_placed_device(0, d_reads, d_refs)
    scores = eng.score_device(0, d_reads, d_refs)
    recs, _ = eng.align_cigar_device(0, d_reads, d_refs, ops_stride=8)
    torch.cuda.synchronize()
    eng.close()
    placed = placed.cpu().numpy().view(hipkernel.placed_dtype()).reshape(-1)
    recs = recs.cpu().numpy().view(hipkernel.aln_dtype()).reshape(-1)
    assert np.array_equal(placed["score"], scores.cpu().numpy().astype(np.int32))
    assert np.array_equal(placed["read_end"], recs["read_end"]) and np.array_equal(placed["ref_end"], recs["ref_end"])
    assert (placed["score"] > 0).sum() > 200


# ---- 7. refusals ----
def test_refusals_and_the_silent_no_op():
    R, F = 64, 128
    reads, refs = _pairs(8, R, F, 1)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()

    def refused(eng, opt, word):
        out = torch.full((8, 3), -7, dtype=torch.int32, device="cuda")
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.score_placed_device(opt, d_reads, d_refs, out=out)
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.score_placed_host(opt, reads, refs)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -7).all() and eng.describe(0, 8)["ran_placed"] == "none"

    eng = hipkernel.Engine(R, F, _scoring("sym"))
    refused(eng, 1, "Smith-Waterman only")
    poisoned = torch.full((8, 3), -7, dtype=torch.int32, device="cuda")
    eng.score_placed_device(2, d_reads, d_refs, out=poisoned)           # opt & 0xF > 1 does nothing, as everywhere
    torch.cuda.synchronize()
    assert (poisoned.cpu().numpy() == -7).all()
    host_out = eng.score_placed_host(2, reads, refs)
    assert not host_out["score"].any()
    eng.set_traceback_policy(1)
    refused(eng, 0, "traceback_policy")
    eng.set_traceback_policy(0)
    eng.set_score_width(32)
    refused(eng, 0, "score_width")
    eng.set_score_width(0)
    _check(_run(eng, reads, refs), placed_ref.placed(reads, refs, _scoring("sym")), "after the refusals")
    eng.set_band_width(16)
    refused(eng, 0, "band_width")
    eng.close()
    eng = hipkernel.Engine(R, F, _scoring("sym", match=600))             # 64 x 600 > 32000: the cells can leave int16
    refused(eng, 0, "int16")
    eng.close()


# ---- 8. host path, streams ----
@pytest.mark.parametrize("chunks", [False, True])
def test_host_path_equals_device_path(monkeypatch, chunks):
    if chunks:
        debug_switches(monkeypatch, chunk_bytes=200000)               # several chunks, more than the pipeline has slots
    R, F = 64, 128
    reads, refs = _pairs(5000, R, F, 12, indel_rate=0.0)
    for form in ("sym", "aff"):
        eng = hipkernel.Engine(R, F, _scoring(form))
        dev = _run(eng, reads, refs)
        for threads in (1, 4):
            got = eng.score_placed_host(0, reads, refs, threads=threads)
            assert got.dtype == hipkernel.placed_dtype() and got.shape == (5000,)
            host_arr = np.stack([got["score"], got["read_end"], got["ref_end"]], axis=1).astype(np.int64)
            _check(host_arr, dev, (form, threads, chunks))
        small = eng.score_placed_host(0, reads[:100], refs[:100], threads=2)        # the direct call
        assert np.array_equal(small["ref_end"].astype(np.int64), dev[:100, 2]) and np.array_equal(small["score"].astype(np.int64), dev[:100, 0])
        eng.close()
    _check(dev[:512], placed_ref.placed(reads[:512], refs[:512], _scoring("aff"), affine=True), "device path")


def test_two_calls_back_to_back_on_a_stream_of_its_own():
    R, F = 150, 500
    ra, fa = _pairs(300, R, F, 21)
    rb, fb = _pairs(300, R, F, 22)
    sc = _scoring("affsym")
    eng = hipkernel.Engine(R, F, sc)
    stream = torch.cuda.Stream()
    d = [torch.from_numpy(x).cuda() for x in (ra, fa, rb, fb)]
    out_a = torch.zeros((300, 3), dtype=torch.int32, device="cuda")
    out_b = torch.zeros((300, 3), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.score_placed_device(0, d[0], d[1], out=out_a, stream=stream)
    eng.score_placed_device(0, d[2], d[3], out=out_b, stream=stream)
    stream.synchronize()
    eng.close()
    _check(out_a.cpu().numpy().astype(np.int64), placed_ref.placed(ra, fa, sc, affine=True), "first call")
    _check(out_b.cpu().numpy().astype(np.int64), placed_ref.placed(rb, fb, sc, affine=True), "second call")
