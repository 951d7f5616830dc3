"""Banded placed Smith-Waterman scores on the GPU (valign_hip_set_band_placed + valign_hip_score_placed_device / _host): the
banded score and the first in-band cell that holds it, from the block chain's sweep, against tests/placed_band_ref.py (numpy,
int64 cells, independent of the library) unless a test says otherwise.  The shapes are the chain's corners -- one strip that is
mostly padding, one row into the second strip, the narrowest band, slopes above and below one, the unit-delay and the
delay-ring form of the kernel -- not the workload."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import placed_band_ref
import placed_ref
from conftest import ROOT, debug_switches
from versalignlib_amd import hipkernel, synth

pytestmark = pytest.mark.gpu

# linear symmetric, linear gap_read != gap_ref, affine symmetric, affine with four scores
FORMS = {"sym": (-3, -3), "lin": (-2, -4), "affsym": (-3, -3, -5, -1, -5, -1), "aff": (-3, -3, -6, -2, -4, -1)}
# (of these (31, 33, 6) alone plans the unit-delay form -- at 1000 x 1000 the first block holds 8 rows, so the window starts do
# not advance evenly and the delay ring runs --; 1024 x 1024 and 528 x 528 are unit-delay over two turns of the cycle)
SHAPES = [(31, 33, 6), (100, 120, 8), (513, 400, 24), (520, 530, 2), (1000, 1000, 64), (1000, 1300, 16), (1300, 1000, 32), (700, 2100, 128),
          (1024, 1024, 64), (528, 528, 32)]
N = 48


def _scoring(form, match=2, mismatch=-1):
    return hipkernel.Scoring.make(match, mismatch, *FORMS[form])


def _affine(form):
    return len(FORMS[form]) > 2


def _pairs(n, R, F, seed, **kw):
    args = dict(sub_rate=0.1, indel_rate=0.01, n_run_frac=0.1, short_frac=0.15, lowercase_frac=0.05, junk_frac=0.05)
    args.update(kw)
    return synth.make_pairs(n, R, F, seed=seed, **args)


def _engine(R, F, sc, band, key=1):
    eng = hipkernel.Engine(R, F, sc)
    eng.set_band_width(band)
    eng.set_band_placed(key)
    return eng


def _run(eng, reads, refs, opt=0):
    out = eng.score_placed_device(opt, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def _check(got, exp, what):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (what, "pairs", bad[:8].tolist(), "got", got[bad[:4]].tolist(), "expected", exp[bad[:4]].tolist())


def _model_plan(R, F, band):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import band_schedule_model as model
    return model.plan(R, F, band // 2, 32, 16)


@functools.lru_cache(maxsize=None)
def _case(R, F, band, form):
    reads, refs = _pairs(N, R, F, 13 * R + F + band)
    exp = placed_band_ref.placed_banded(reads, refs, band, _scoring(form), affine=_affine(form))
    exp.setflags(write=False)
    return reads, refs, exp


# ---- 1. parity on the chain's corners ----
def test_the_shapes_hold_both_forms_of_the_kernel():
    units = [_model_plan(R, F, band)["unit"] for R, F, band in SHAPES]
    assert any(units) and not all(units), units
    assert _model_plan(31, 33, 6)["unit"] and _model_plan(1024, 1024, 64)["unit"] and _model_plan(528, 528, 32)["unit"]
    assert not _model_plan(1000, 1000, 64)["unit"] and not _model_plan(1000, 1300, 16)["unit"]


@pytest.mark.parametrize("R,F,band", SHAPES)
def test_parity_with_the_numpy_statement(R, F, band):
    unit = _model_plan(R, F, band)["unit"]           # (on the CPU, before any GPU call)
    for form in FORMS:
        reads, refs, exp = _case(R, F, band, form)
        eng = _engine(R, F, _scoring(form), band)
        d = eng.describe(0, N)
        assert (d["band_block_rows"], d["band_col_align"], d["band_placed"]) == (16, 1, 1), d
        got = _run(eng, reads, refs)
        d = eng.describe(0, N)
        eng.close()
        assert d["ran_placed"] == "chain", (R, F, band, form, d["ran_placed"])
        _check(got, exp, (R, F, band, form, "unit" if unit else "ring"))
        assert (exp[:, 0] > 0).sum() > N // 2


# ---- 2. ties, built on purpose ----
# An N background, motifs placed by hand, and a scoring under which no path through two motifs beats one: a mismatch or a gap
# base costs more than two matches give.  A motif of m bases whose last cell is (row e, column c) scores m * match there; the
# column is given relative to the band's centre line c = e * F // R + off.
def _tie_scoring(form, match=2):
    g = -(2 * match + 1)
    return hipkernel.Scoring.make(match, g, g, g) if form == "sym" else hipkernel.Scoring.make(match, g, g, g, g - 3, g, g - 1, g)


def _motifs(rng, m):
    letters = np.frombuffer(b"ACGT", np.uint8)
    a = rng.choice(letters, m)
    b = a.copy()
    b[::2] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(letters, a[::2])]      # differs from a at every other base
    return a, b


TIE_M = 6          # bases per motif: two motifs fit into the rows of one block


def _tie_batches(R, F):
    """name -> (reads, refs, [(read_end, ref_end) per pair]); 16-row blocks: block of row r = (r + pad) // 16, lane = block % 32"""
    pad = -R % 512
    rng = np.random.default_rng(R + F)
    m = TIE_M
    out = {}

    def blank(n):
        return np.full((n, R), ord("N"), np.uint8), np.full((n, F), ord("N"), np.uint8)

    def put(reads, refs, p, motif, e, off):
        c = e * F // R + off
        assert e - m + 1 >= 0 and c - m + 1 >= 0 and c < F and e < R
        reads[p, e - m + 1:e + 1] = motif
        refs[p, c - m + 1:c + 1] = motif
        return e + 1, c + 1

    def row_at(block, q):
        return block * 16 + q - pad

    n = 8
    first_block = pad // 16 + 3
    # (a) the same row at two columns: the earlier column
    reads, refs = blank(n)
    where = []
    for p in range(n):
        a, _ = _motifs(rng, m)
        e = row_at(first_block + 5 * p, p % 16)
        where.append(put(reads, refs, p, a, e, -30 - p))
        put(reads, refs, p, a, e, 25 + p)
    out["one_row_two_columns"] = (reads, refs, where)
    # (b) two rows of one block, the later row in the earlier column; (c) blocks b and b + 32 -- the same lane, 512 rows apart,
    # the later block's row nearer the top of its block (the greater key, were the lane's key not closed at the event);
    # (d) rows in different lanes, again with the later one nearer the top of its block
    for name, dblock, q1, q2 in (("two_rows_of_one_block", 0, 4, 11), ("same_lane_512_rows_apart", 32, 10, 3), ("two_lanes", 3, 12, 2)):
        reads, refs = blank(n)
        where = []
        for p in range(n):
            a, b = _motifs(rng, m)
            blk = first_block + 2 * p
            side = 1 if dblock == 0 else -1           # (one block: the later row lies in the earlier column)
            where.append(put(reads, refs, p, a, row_at(blk, q1), side * (20 + p)))
            late = put(reads, refs, p, b, row_at(blk + dblock, q2), -side * (25 + p))
            assert late[0] - m >= where[-1][0] and abs(late[1] - where[-1][1]) >= m          # (the motifs share no row and no column)
            assert dblock or late[1] < where[-1][1]
        out[name] = (reads, refs, where)
    # (e) the same pair in both halves of a lane group (pairs 2 k and 2 k + 1 take turns on one group's registers)
    reads, refs = blank(n)
    where = []
    for p in range(0, n, 2):
        a, b = _motifs(rng, m)
        blk = first_block + 7 * p
        for h in (0, 1):
            where.append(put(reads, refs, p + h, a, row_at(blk, 9), 11))
            put(reads, refs, p + h, b, row_at(blk + 1, 1), -11)
    out["both_halves"] = (reads, refs, where)
    return out


@pytest.mark.parametrize("R,F,band", [(1024, 1024, 256), (1000, 1300, 200)])
@pytest.mark.parametrize("form", ["sym", "aff"])
def test_ties(form, R, F, band):
    assert R >= 600 and _model_plan(R, F, band)["unit"] == (R == F)          # the unit-delay form and the delay ring
    sc = _tie_scoring(form)
    eng = _engine(R, F, sc, band)
    for name, (reads, refs, where) in _tie_batches(R, F).items():
        got = _run(eng, reads, refs)
        assert eng.describe(0, len(reads))["ran_placed"] == "chain"
        exp = placed_band_ref.placed_banded(reads, refs, band, sc, affine=form == "aff")
        _check(got, exp, (name, form, R, F))
        for p in range(len(reads)):           # ... and the construction says where, independently of any fill
            assert tuple(got[p]) == (2 * TIE_M,) + where[p], (name, p, got[p].tolist(), where[p])
    eng.close()


# ---- 3. pair counts: quads of pairs, the last one short ----
@pytest.mark.parametrize("form", ["sym", "aff"])
def test_pair_counts_and_nothing_written_beyond(form):
    R, F, band = 513, 400, 24
    reads, refs = _pairs(67, R, F, 99)
    sc = _scoring(form)
    exp = placed_band_ref.placed_banded(reads, refs, band, sc, affine=_affine(form))
    eng = _engine(R, F, sc, band)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    for n in (1, 2, 3, 5, 67):
        buf = torch.full((n + 9, 3), -7, dtype=torch.int32, device="cuda")
        eng.score_placed_device(0, d_reads[:n], d_refs[:n], out=buf[:n])
        torch.cuda.synchronize()
        got = buf.cpu().numpy().astype(np.int64)
        _check(got[:n], exp[:n], (form, n))
        assert (got[n:] == -7).all(), (form, n)
    eng.close()


# ---- 4. consistency on one engine ----
@pytest.mark.parametrize("R,F,band", [(1024, 1024, 64), (513, 400, 24)])
@pytest.mark.parametrize("form", ["sym", "aff"])
def test_score_is_the_banded_score_and_empty_pairs_are_zero(R, F, band, form):
    reads, refs = _pairs(N, R, F, R + band)
    reads[5] = ord("N")
    refs[9] = ord("n")
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    eng = _engine(R, F, _scoring(form), band)
    placed = eng.score_placed_device(0, d_reads, d_refs)
    scores = eng.score_device(0, d_reads, d_refs)
    torch.cuda.synchronize()
    eng.close()
    placed = placed.cpu().numpy()
    scores = scores.cpu().numpy().astype(np.int32)
    assert scores.max() < 32767 and np.array_equal(placed[:, 0], scores)
    assert not placed[5].any() and not placed[9].any() and (placed[:, 0] > 0).sum() >= N - 6


# (a band that wide makes every window the whole row; the chain plans it while its rings fit: with affine gaps -- a second
# delay ring -- up to F + max(R, F) of about 1 000, with linear gaps further: 1025 x 200 is there for the strips' route)
@pytest.mark.parametrize("R,F,forms,route", [(150, 300, "sym lin affsym aff", ("key", "rows")), (300, 400, "sym lin affsym aff", ("key", "rows")),
                                             (1025, 200, "sym lin", ("strip",))])
def test_a_band_wider_than_the_matrix_is_the_unbanded_route(R, F, forms, route):
    reads, refs = _pairs(N, R, F, R + 3)
    for form in forms.split():
        sc = _scoring(form)
        eng = hipkernel.Engine(R, F, sc)
        unbanded = _run(eng, reads, refs)
        assert eng.describe(0, N)["ran_placed"] in route
        eng.close()
        eng = _engine(R, F, sc, 2 * max(R, F))
        banded = _run(eng, reads, refs)
        assert eng.describe(0, N)["ran_placed"] == "chain"
        eng.close()
        _check(banded, unbanded, (R, F, form))
        _check(banded, placed_ref.placed(reads, refs, sc, affine=_affine(form)), (R, F, form, "numpy"))


def test_affine_gaps_where_only_the_linear_plan_fits_are_refused():
    """1025 x 200 under a band of 2050: the delay rings are 64 slots deep, and the second ring of affine gaps does not fit"""
    R, F = 1025, 200
    reads, refs = _pairs(4, R, F, 5)
    eng = _engine(R, F, _scoring("affsym"), 2 * R)
    out = torch.full((4, 3), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(hipkernel.HipKernelError, match="band_placed.*plan"):
        eng.score_placed_device(0, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda(), out=out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all() and eng.describe(0, 4)["ran_placed"] == "none"
    eng.close()


# ---- 5. refusals and non-effects ----
def test_refusals_and_what_the_key_leaves_alone():
    R, F, band = 200, 260, 16
    reads, refs = _pairs(8, R, F, 1)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    sc = _scoring("sym")

    def refused(eng, opt, word, r=reads, f=refs):
        out = torch.full((len(r), 3), -7, dtype=torch.int32, device="cuda")
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.score_placed_device(opt, torch.from_numpy(r).cuda(), torch.from_numpy(f).cuda(), out=out)
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.score_placed_host(opt, r, f)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -7).all() and eng.describe(0, 8)["ran_placed"] == "none"

    eng = hipkernel.Engine(R, F, sc)
    for bad in (2, -1):
        with pytest.raises(hipkernel.HipKernelError, match="band_placed must be 0 or 1"):
            eng.set_band_placed(bad)
    assert eng.describe(0, 8)["band_placed"] == 0
    # key 1 without a band: the unbanded route, the unbanded records
    eng.set_band_placed(1)
    assert eng.describe(0, 8)["band_placed"] == 1
    _check(_run(eng, reads, refs), placed_ref.placed(reads, refs, sc), "key on, no band")
    assert eng.describe(0, 8)["ran_placed"] in ("key", "rows")
    # key 0 with a band: refused as ever
    eng.set_band_placed(0)
    eng.set_band_width(band)
    refused(eng, 0, "band_width")
    # key 1 with a band: the NW variant and traceback_policy = 1 are refused, score_width = 32 runs
    eng.set_band_placed(1)
    refused(eng, 1, "Smith-Waterman only")
    eng.set_traceback_policy(1)
    refused(eng, 0, "traceback_policy")
    eng.set_traceback_policy(0)
    exp = placed_band_ref.placed_banded(reads, refs, band, sc)
    for width in (32, 16, 0):
        eng.set_score_width(width)
        _check(_run(eng, reads, refs), exp, ("score_width", width))
        assert eng.describe(0, 8)["ran_placed"] == "chain"
    # ... and back without the band: the unbanded route again
    eng.set_band_width(0)
    _check(_run(eng, reads, refs), placed_ref.placed(reads, refs, sc), "band off again")
    eng.close()
    # a shape whose plan is unusable (a reference ring beyond 2048 columns: tests/long_plan_check.cpp): refused, never stripped
    R2, F2 = 2, 3853
    r2, f2 = _pairs(8, R2, F2, 2, indel_rate=0.0, short_frac=0.0)
    eng = _engine(R2, F2, sc, 64)
    refused(eng, 0, "band_placed", r2, f2)
    with pytest.raises(hipkernel.HipKernelError, match="plan"):
        eng.score_placed_host(0, r2, f2)
    eng.close()


def test_long_reads_stay_on_the_chain():
    """2 100 rows: unbanded placed scores would take the strips; under band_placed the route is the chain whatever the read"""
    R, F, band = 2100, 2000, 48
    reads, refs = _pairs(6, R, F, 17, indel_rate=0.0)
    sc = _scoring("affsym")
    eng = _engine(R, F, sc, band)
    got = _run(eng, reads, refs)
    assert eng.describe(0, 6)["ran_placed"] == "chain"
    eng.close()
    _check(got, placed_band_ref.placed_banded(reads, refs, band, sc, affine=True), "2100 x 2000")


# ---- 6. host path ----
@pytest.mark.parametrize("chunks", [False, True])
def test_host_path_equals_device_path(monkeypatch, chunks):
    if chunks:
        debug_switches(monkeypatch, chunk_bytes=200000)               # several chunks, more than the pipeline has slots
    R, F, band = 100, 120, 8
    reads, refs = _pairs(5000, R, F, 12, indel_rate=0.0)
    for form in ("sym", "aff"):
        eng = _engine(R, F, _scoring(form), band)
        dev = _run(eng, reads, refs)
        for threads in (1, 4):
            got = eng.score_placed_host(0, reads, refs, threads=threads)
            assert got.dtype == hipkernel.placed_dtype() and got.shape == (5000,)
            host_arr = np.stack([got["score"], got["read_end"], got["ref_end"]], axis=1).astype(np.int64)
            _check(host_arr, dev, (form, threads, chunks))
        assert eng.describe(0, 5000)["ran_placed"] == "chain"
        small = eng.score_placed_host(0, reads[:100], refs[:100], threads=2)        # the direct call
        assert eng.describe(0, 100)["direct_call"] == 1 and eng.describe(0, 100)["ran_placed"] == "chain"
        small_arr = np.stack([small["score"], small["read_end"], small["ref_end"]], axis=1).astype(np.int64)
        _check(small_arr, dev[:100], (form, "direct"))
        eng.close()
    _check(dev[:256], placed_band_ref.placed_banded(reads[:256], refs[:256], band, _scoring("aff"), affine=True), "device path")
