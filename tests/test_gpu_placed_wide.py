"""Placed and spanned Smith-Waterman scores on int32 cells (key placed_wide; valign_hip_set_placed_wide) on the GPU, against
tests/placed_ref.py and tests/span_ref.py (numpy, int64 cells, independent of the library -- exact for these scores) unless a
test says otherwise.

The sweep runs in strips of 512 rows (8 rows per lane, 64 lanes), padding rows on top of strip 0: the shapes are the smallest
that put the maximum in a padded strip, across strips, in one lane, in two lanes and in two strips.  The rule that picks the
route (placed_choice, cell_rules.h) is restated in `_predict` so that describe()["ran_placed"] is checked against a
prediction, not against itself."""
import functools

import numpy as np
import pytest
import torch

import placed_ref
import span_ref
from conftest import debug_switches
from versalignlib_amd import hipkernel, synth

pytestmark = pytest.mark.gpu

# linear symmetric, linear gap_read != gap_ref, affine symmetric, affine with four scores
FORMS = {"sym": (-3, -3), "lin": (-2, -4), "affsym": (-3, -3, -5, -1, -5, -1), "aff": (-3, -3, -6, -2, -4, -1)}
REFUSED_32 = "placed scores are not built for score_width = 32 \\(int32 cells\\)"
REFUSED_16 = "placed scores run on int16 cells: shape x scoring can leave their range"


def _scoring(form, match=2, mismatch=-1):
    return hipkernel.Scoring.make(match, mismatch, *FORMS[form])


def _affine(form):
    return len(FORMS[form]) > 2


def _pairs(n, R, F, seed, **kw):
    args = dict(sub_rate=0.1, indel_rate=0.02, n_run_frac=0.1, short_frac=0.1, lowercase_frac=0.05, junk_frac=0.04)
    args.update(kw)
    return synth.make_pairs(n, R, F, seed=seed, **args)


def _engine(R, F, sc, width=32, wide=1):
    eng = hipkernel.Engine(R, F, sc)
    eng.set_score_width(width)
    eng.set_placed_wide(wide)
    return eng


def _run(eng, reads, refs, opt=0):
    out = eng.score_placed_device(opt, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def _span(eng, reads, refs, opt=0):
    out = eng.score_span_device(opt, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def _check(got, exp, what):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (what, "pairs", bad[:8].tolist(), "got", got[bad[:4]].tolist(), "expected", exp[bad[:4]].tolist())


@functools.lru_cache(maxsize=None)
def _case(R, F, form, seed, n=9, match=2):
    """the reference of a case, computed once and shared (read-only)"""
    reads, refs = _pairs(n, R, F, seed)
    sc = _scoring(form, match)
    placed = placed_ref.placed(reads, refs, sc, affine=_affine(form))
    spans = span_ref.spans(reads, refs, sc, affine=_affine(form), chunk=16)
    for a in (reads, refs, placed, spans):
        a.setflags(write=False)
    return reads, refs, placed, spans


SMALL = [(12, 20), (70, 90), (150, 5), (511, 64), (512, 129)]


# ---- 1. one strip, padding rows on top; score_width = 32 with ordinary scores; an odd count and a last wave of one pair ----
@pytest.mark.parametrize("R,F", SMALL)
def test_single_strip_with_padding_rows(R, F):
    for form in FORMS:
        reads, refs, exp, _ = _case(R, F, form, 7 * R + F)
        eng = _engine(R, F, _scoring(form))
        for n in (1, 2, 9):
            got = _run(eng, reads[:n], refs[:n])
            assert eng.describe(0, n)["ran_placed"] == "wide", (R, F, form, n)
            _check(got, exp[:n], (R, F, form, n))
        eng.close()
        assert (exp[:, 0] > 0).any()


# ---- 2. across strips: boundary rows handed on, H and (affine) F ----
def _straddling(n, R, F, seed):
    """random pairs whose read holds a copy of a reference window (pair 0: exact, in a read of N otherwise; the others: one base
    in ten replaced) across the last seam, row R - 512 -> reads, refs, seam"""
    reads, refs = _pairs(n, R, F, seed, short_frac=0.0)
    rng = np.random.default_rng(seed)
    L, seam = min(R, F) - 10, R - 512
    start = min(max(seam - L // 2, 0), R - L)
    for p in range(n):
        window = rng.choice(np.frombuffer(b"ACGT", np.uint8), L)
        refs[p, 5:5 + L] = window
        if p:
            window = np.where(rng.random(L) < 0.1, rng.choice(np.frombuffer(b"ACGT", np.uint8), L), window)
        else:
            reads[p] = ord("N")
        reads[p, start:start + L] = window
    return reads, refs, seam


@pytest.mark.parametrize("R", [513, 600, 1024, 1025])
@pytest.mark.parametrize("F", [90, 700])
def test_across_strips(R, F):
    n = 5
    reads, refs, seam = _straddling(n, R, F, 3 * R + F)
    for form in ("lin", "aff"):
        sc = _scoring(form)
        exp = placed_ref.placed(reads, refs, sc, affine=_affine(form))
        eng = _engine(R, F, sc)
        got = _run(eng, reads, refs)
        assert eng.describe(0, n)["ran_placed"] == "wide"
        eng.close()
        _check(got, exp, (R, F, form))
        # a score of s at match 2 covers at least s / 2 read rows: such an alignment ends below the seam and begins above it
        assert ((exp[:, 1] > seam) & (exp[:, 0] > 2 * (exp[:, 1] - seam))).any(), (exp.tolist(), seam)


# ---- 3. out of int16 by the scoring, score_width = 0: scores above 32767, and above 65535 (EndCell.pad carries real bits) ----
@pytest.mark.parametrize("match,top", [(300, 32767), (500, 65535)])
def test_scores_beyond_int16(match, top):
    R, F = 150, 200
    reads, refs = _pairs(9, R, F, match)
    reads[:4], refs[:4] = synth.make_pairs(4, R, F, seed=match + 1, sub_rate=0.0, indel_rate=0.0, n_run_frac=0.0, short_frac=0.0)      # identical pairs
    for form in FORMS:
        sc = hipkernel.Scoring.make(match, -4, *[6 * g for g in FORMS[form]])
        exp = placed_ref.placed(reads, refs, sc, affine=_affine(form))
        assert exp[:4, 0].min() > top and exp[:4, 0].max() == R * match, exp[:4, 0]
        eng = _engine(R, F, sc, width=0)
        got = _run(eng, reads, refs)
        assert eng.describe(0, 9)["ran_placed"] == "wide"
        _check(got, exp, (match, form))
        _check(_span(eng, reads, refs), span_ref.spans(reads, refs, sc, affine=_affine(form)), ("spanned", match, form))
        assert eng.describe(0, 9)["ran_span"] == "wide/wide"
        eng.close()


# ---- 4. ties, constructed: R = 600 is strip 0 = rows [0, 88) (424 padding rows on top) and strip 1 = rows [88, 600) ----
TR, TF = 600, 700
# per pair: the half-open read ranges and ref ranges that hold the motif (the last case: 41 bases in the second read range and in
# the reference), and the record
TIES = [
    ([(20, 60), (300, 340)], [(30, 70)], (80000, 60, 70)),             # the maximum ties in strip 0 and strip 1: the earlier strip wins
    ([(100, 140), (300, 340)], [(30, 70)], (80000, 140, 70)),          # two rows in different lanes of strip 1: the earlier row wins
    ([(300, 340)], [(30, 70), (400, 440)], (80000, 340, 70)),          # one row, two columns: the first column wins
    ([(20, 60)], [(30, 70)], (80000, 60, 70)),                         # one copy
    ([(20, 60), (300, 341)], [(30, 71)], (82000, 341, 71)),            # the later strip strictly larger by one matching base: it wins
]


def _tie_scoring(affine):
    return hipkernel.Scoring.make(2000, -1500, -2500, -2500, -3000, -500, -3000, -500) if affine else hipkernel.Scoring.make(2000, -1500, -2500, -2500)


@functools.lru_cache(maxsize=None)
def _tie_batch():
    rng = np.random.default_rng(600700)
    reads = np.full((len(TIES), TR), ord("N"), np.uint8)
    refs = np.full((len(TIES), TF), ord("N"), np.uint8)
    for p, (read_at, ref_at, _) in enumerate(TIES):
        motif = rng.choice(np.frombuffer(b"ACGT", np.uint8), 41)
        for lo, hi in read_at:
            reads[p, lo:hi] = motif[:hi - lo]
        for lo, hi in ref_at:
            refs[p, lo:hi] = motif[:hi - lo]
    reads.setflags(write=False)
    refs.setflags(write=False)
    return reads, refs


@pytest.mark.parametrize("affine", [False, True])
def test_ties(affine):
    reads, refs = _tie_batch()
    sc = _tie_scoring(affine)
    exp = placed_ref.placed(reads, refs, sc, affine=affine)
    for p, (_, _, rec) in enumerate(TIES):             # the construction says where, independently of any fill -- and the numpy fill agrees
        assert tuple(exp[p]) == rec, (p, exp[p].tolist(), rec)
    eng = _engine(TR, TF, sc, width=0)                 # 600 x 2000 leaves int16 by itself
    got = _run(eng, reads, refs)
    assert eng.describe(0, len(TIES))["ran_placed"] == "wide"
    _check(got, exp, ("ties", affine))
    # spanned: the begin cells by the reversed-sweep rule
    spans = _span(eng, reads, refs)
    assert eng.describe(0, len(TIES))["ran_span"].startswith("wide/")
    eng.close()
    _check(spans, span_ref.spans(reads, refs, sc, affine=affine), ("spanned ties", affine))
    for p, (_, _, rec) in enumerate(TIES):
        m = rec[0] // 2000
        assert tuple(spans[p]) == (rec[0], rec[1] - m, rec[1], rec[2] - m, rec[2]), (p, spans[p].tolist())


# ---- 5. empty pairs ----
def test_empty_pairs():
    R, F = 600, 90
    reads, refs = _pairs(6, R, F, 5)
    reads[::2] = ord("N")
    for form in ("sym", "aff"):
        sc = _scoring(form)
        eng = _engine(R, F, sc)
        got = _run(eng, reads, refs)
        spans = _span(eng, reads, refs)
        eng.close()
        _check(got, placed_ref.placed(reads, refs, sc, affine=_affine(form)), ("empty", form))
        assert not got[::2].any() and got[1::2, 0].all() and got.shape == (6, 3)
        assert not spans[::2].any() and spans.shape == (6, 5)
        _check(spans, span_ref.spans(reads, refs, sc, affine=_affine(form)), ("empty spans", form))


# ---- 6. agreement with what already runs ----
@pytest.mark.parametrize("R,F,match,route", [(150, 500, 2, "key"), (150, 500, 100, "rows"), (1025, 130, 2, "strip")])
def test_equals_the_int16_routes_in_range(R, F, match, route):
    reads, refs = _pairs(130, R, F, R + match)
    for form in ("sym", "aff"):
        sc = _scoring(form, match)
        eng = hipkernel.Engine(R, F, sc)
        narrow = _run(eng, reads, refs)
        assert eng.describe(0, 130)["ran_placed"] == route and eng.describe(0, 130)["placed_wide"] == 0
        eng.set_placed_wide(1)
        assert np.array_equal(_run(eng, reads, refs), narrow) and eng.describe(0, 130)["ran_placed"] == route       # in range: the key changes nothing
        eng.set_score_width(16)
        assert np.array_equal(_run(eng, reads, refs), narrow) and eng.describe(0, 130)["ran_placed"] == route
        eng.set_score_width(32)
        wide = _run(eng, reads, refs)
        assert eng.describe(0, 130)["ran_placed"] == "wide" and eng.describe(0, 130)["placed_wide"] == 1
        _check(wide, narrow, (R, F, match, form))
        # ... and the int32 score sweep's scores
        scores = eng.score_device(0, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda())
        torch.cuda.synchronize()
        eng.close()
        scores = scores.cpu().numpy().astype(np.int64)
        assert scores.max() < 32767 and np.array_equal(wide[:, 0], scores)
        assert (wide[:, 0] > 0).sum() > 100


@pytest.mark.parametrize("form", ["sym", "aff"])
def test_equals_the_cigar_records_of_the_same_out_of_range_call(form):
    R, F, match = 150, 200, 300
    reads, refs = _pairs(64, R, F, 31)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    eng = _engine(R, F, hipkernel.Scoring.make(match, -4, *[6 * g for g in FORMS[form]]), width=0)
    placed = eng.score_placed_device(0, d_reads, d_refs)
    recs, _ = eng.align_cigar_device(0, d_reads, d_refs, ops_stride=8)
    scores = eng.score_device(0, d_reads, d_refs)
    torch.cuda.synchronize()
    d = eng.describe(0, 64)
    eng.close()
    assert d["ran_placed"] == "wide" and d["ran_align_fill"] == "strip_wide", d
    placed = placed.cpu().numpy().view(hipkernel.placed_dtype()).reshape(-1)
    recs = recs.cpu().numpy().view(hipkernel.aln_dtype()).reshape(-1)
    for k in ("score", "read_end", "ref_end"):
        assert np.array_equal(placed[k], recs[k]), k
    scores = scores.cpu().numpy().astype(np.int64)
    below = scores < 32767
    assert below.any() and (~below).any() and np.array_equal(placed["score"][below], scores[below]) and (placed["score"][~below] >= 32767).all()


# ---- 7. spanned scores ----
@pytest.mark.parametrize("R,F", SMALL)
def test_spanned(R, F):
    for form in FORMS:
        reads, refs, placed, exp = _case(R, F, form, 7 * R + F)
        eng = _engine(R, F, _scoring(form))
        for n in (1, 9):
            got = _span(eng, reads[:n], refs[:n])
            d = eng.describe(0, n)
            assert d["ran_span"] == "wide/wide" and d["ran_placed"] == "wide", d["ran_span"]
            _check(got, exp[:n], (R, F, form, n))
        host = eng.score_span_host(0, reads, refs, threads=2)
        eng.close()
        _check(np.stack([host[k] for k in hipkernel.span_dtype().names], axis=1).astype(np.int64), exp, ("host", R, F, form))
        _check(exp[:, [0, 2, 4]], placed, "the two references agree")


def test_spanned_across_strips():
    R, F = 1025, 700
    reads, refs, _ = _straddling(5, R, F, 77)
    sc = _scoring("aff")
    eng = _engine(R, F, sc)
    got = _span(eng, reads, refs)
    assert eng.describe(0, 5)["ran_span"] == "wide/wide"
    eng.close()
    _check(got, span_ref.spans(reads, refs, sc, affine=True), "spanned, three strips")


# ---- 8. key handling ----
def test_key_handling_and_refusals():
    R, F = 64, 128
    reads, refs = _pairs(8, R, F, 1)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()

    def refused(eng, opt, text):
        out = torch.full((8, 3), -7, dtype=torch.int32, device="cuda")
        spans = torch.full((8, 5), -7, dtype=torch.int32, device="cuda")
        with pytest.raises(hipkernel.HipKernelError, match=text):
            eng.score_placed_device(opt, d_reads, d_refs, out=out)
        with pytest.raises(hipkernel.HipKernelError, match=text):
            eng.score_placed_host(opt, reads, refs)
        if "band_width" not in text:            # (spanned scores name the band in a text of their own)
            with pytest.raises(hipkernel.HipKernelError, match=text):
                eng.score_span_device(opt, d_reads, d_refs, out=spans)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -7).all() and (spans.cpu().numpy() == -7).all() and eng.describe(0, 8)["ran_placed"] == "none"

    eng = hipkernel.Engine(R, F, _scoring("sym"))
    assert eng.describe(0, 8)["placed_wide"] == 0 and eng.describe(0, 8)["ran_placed"] == "none"
    for value in (2, -1):
        with pytest.raises(hipkernel.HipKernelError, match="placed_wide must be 0 or 1"):
            eng.set_placed_wide(value)
    assert eng.describe(0, 8)["placed_wide"] == 0
    # key off: both refusals with today's texts
    eng.set_score_width(32)
    refused(eng, 0, REFUSED_32)
    eng.set_placed_wide(1)
    assert eng.describe(0, 8)["placed_wide"] == 1
    _check(_run(eng, reads, refs), placed_ref.placed(reads, refs, _scoring("sym")), "key on")
    assert eng.describe(0, 8)["ran_placed"] == "wide"
    # the NW variant, traceback_policy = 1 and a band: refused as ever with the key on
    refused(eng, 1, "Smith-Waterman only")
    eng.set_traceback_policy(1)
    refused(eng, 0, "placed scores are not built for traceback_policy = 1")
    eng.set_traceback_policy(0)
    eng.set_band_width(16)
    refused(eng, 0, "placed scores are not built for band_width > 0")
    with pytest.raises(hipkernel.HipKernelError, match="spanned scores are not built for band_width > 0"):
        eng.score_span_device(0, d_reads, d_refs)
    eng.set_band_width(0)
    eng.set_placed_wide(0)
    refused(eng, 0, REFUSED_32)
    eng.close()
    # out of int16 by the scoring: key off refused with today's text; score_width = 16 stays refused with the key on
    eng = hipkernel.Engine(R, F, _scoring("sym", match=600))
    refused(eng, 0, REFUSED_16)
    eng.set_placed_wide(1)
    eng.set_score_width(16)
    refused(eng, 0, REFUSED_16)
    eng.set_score_width(0)
    _check(_run(eng, reads, refs), placed_ref.placed(reads, refs, _scoring("sym", match=600)), "64 x 128 at match 600")
    assert eng.describe(0, 8)["ran_placed"] == "wide"
    eng.close()


def test_int32_range_edge():
    """(R + F + 2) x |score| = 2^28 at 4100 x 4100: match 32728 is the last that runs, 32729 is refused by name"""
    R = F = 4100
    last = ((1 << 28) - 1) // (R + F + 2)
    assert last == 32728
    reads, refs = synth.make_pairs(2, R, F, seed=4, sub_rate=0.0, indel_rate=0.0, n_run_frac=0.0, short_frac=0.0)      # identical pairs of ACGT
    assert np.array_equal(reads, refs) and np.isin(reads, np.frombuffer(b"ACGT", np.uint8)).all()
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    eng = _engine(R, F, hipkernel.Scoring.make(last + 1, -1, -3, -3), width=0)
    with pytest.raises(hipkernel.HipKernelError, match="^placed_wide: shape x scoring can leave the int32 range"):
        eng.score_placed_device(0, d_reads, d_refs)
    with pytest.raises(hipkernel.HipKernelError, match="^placed_wide: "):
        eng.score_span_device(0, d_reads, d_refs)
    assert eng.describe(0, 2)["ran_placed"] == "none"
    eng.close()
    eng = _engine(R, F, hipkernel.Scoring.make(last, -1, -3, -3), width=0)
    got = eng.score_placed_device(0, d_reads, d_refs)
    torch.cuda.synchronize()
    assert eng.describe(0, 2)["ran_placed"] == "wide"
    eng.close()
    # an identical pair's only maximum is the whole diagonal: the largest value the rule lets through, exact
    assert got.cpu().numpy().tolist() == [[R * last, R, F]] * 2


# ---- 9. host path, chunks, streams ----
@pytest.mark.parametrize("chunks", [False, True])
def test_host_path_equals_device_path(monkeypatch, chunks):
    if chunks:
        debug_switches(monkeypatch, chunk_bytes=200000)               # several chunks, more than the pipeline has slots
    R, F = 70, 90
    reads, refs = _pairs(5001, R, F, 12, indel_rate=0.0)
    for form in ("sym", "aff"):
        eng = _engine(R, F, _scoring(form))
        dev = _run(eng, reads, refs)
        got = eng.score_placed_host(0, reads, refs, threads=4)
        assert got.dtype == hipkernel.placed_dtype() and got.shape == (5001,) and eng.describe(0, 1)["ran_placed"] == "wide"
        _check(np.stack([got["score"], got["read_end"], got["ref_end"]], axis=1).astype(np.int64), dev, (form, chunks))
        small = eng.score_placed_host(0, reads[:99], refs[:99], threads=2)        # the direct call
        _check(np.stack([small["score"], small["read_end"], small["ref_end"]], axis=1).astype(np.int64), dev[:99], (form, "direct"))
        eng.close()
    _check(dev[:256], placed_ref.placed(reads[:256], refs[:256], _scoring("aff"), affine=True), "device path")


def test_two_calls_back_to_back_reuse_and_regrow_the_scratch():
    R, F = 600, 90
    ra, fa = _pairs(7, R, F, 21)
    rb, fb = _pairs(40, R, F, 22)
    sc = _scoring("aff")
    eng = _engine(R, F, sc)
    stream = torch.cuda.Stream()
    d = [torch.from_numpy(x).cuda() for x in (ra, fa, rb, fb)]
    outs = [torch.zeros((n, 3), dtype=torch.int32, device="cuda") for n in (7, 40, 7)]
    torch.cuda.synchronize()
    eng.score_placed_device(0, d[0], d[1], out=outs[0], stream=stream)
    eng.score_placed_device(0, d[2], d[3], out=outs[1], stream=stream)       # more pairs: the scratch regrows behind the first call
    eng.score_placed_device(0, d[0], d[1], out=outs[2], stream=stream)       # fewer again: reused
    stream.synchronize()
    assert eng.describe(0, 7)["placed_scratch_bytes"] > 0
    eng.close()
    _check(outs[0].cpu().numpy().astype(np.int64), placed_ref.placed(ra, fa, sc, affine=True), "first call")
    _check(outs[1].cpu().numpy().astype(np.int64), placed_ref.placed(rb, fb, sc, affine=True), "second call")
    assert np.array_equal(outs[2].cpu().numpy(), outs[0].cpu().numpy())


def test_strip_and_wide_calls_share_one_engine():
    """the int16 strips and the int32 sweep keep their rows in the same engine-owned scratch: either order, either size"""
    R, F = 1025, 130
    reads, refs = _pairs(12, R, F, 9)
    sc = _scoring("lin")
    exp = placed_ref.placed(reads, refs, sc)
    eng = hipkernel.Engine(R, F, sc)
    eng.set_placed_wide(1)
    for width, route, n in ((32, "wide", 12), (0, "strip", 12), (32, "wide", 3), (0, "strip", 5)):
        eng.set_score_width(width)
        _check(_run(eng, reads[:n], refs[:n]), exp[:n], (width, n))
        assert eng.describe(0, n)["ran_placed"] == route
    eng.close()


# ---- 9b. a strip sweep cut into several scratch chunks, the last one short and odd: the scratch is laid out for the waves of a
# full chunk, the last launch runs fewer ----
CR, CF, CAP_MB = 1025, 700, 1
CHUNKED = {"strip": (0, 299), "wide": (32, 151)}           # route: score_width, pairs


def _chunk_pairs(width):
    """pairs of one scratch chunk under the cap (strip_plan.h, ckpt_plan.h, restated): per pair-of-pairs two row sets that
    ping-pong, each an H and an F row (affine) of row_dwords dwords, and on int32 cells one such row per pair"""
    row_dwords = ((CF + 71) // 64 + 2) * 64
    row_sets = 2 * (2 if width == 32 else 1)
    return (CAP_MB << 20) // (2 * row_sets * row_dwords * 4) * 2


def _chunked_engine(width, capped):
    eng = _engine(CR, CF, _scoring("aff"), width=width)
    if capped:
        eng.set_pointer_scratch_cap_mb(CAP_MB)
    return eng


def _records(host):
    return np.stack([host[k] for k in host.dtype.names], axis=1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _chunked_case():
    """the batch, the reference of its first 16 pairs and the uncapped engines' records of every route, computed once (read-only)"""
    reads, refs = _pairs(299, CR, CF, 1616)
    out = {"reads": reads, "refs": refs, "ref16": placed_ref.placed(reads[:16], refs[:16], _scoring("aff"), affine=True)}
    for route, (width, n) in CHUNKED.items():
        eng = _chunked_engine(width, capped=False)
        out[route] = _run(eng, reads[:n], refs[:n])
        out[route, "scratch"] = eng.describe(0, n)["placed_scratch_bytes"]
        eng.close()
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def test_chunk_counts_of_the_capped_sweeps():
    assert CF + 135 <= ((CF + 71) // 64 + 2) * 64 == 896 and (_chunk_pairs(0), _chunk_pairs(32)) == (146, 72)
    for width, n in CHUNKED.values():
        chunk = _chunk_pairs(width)
        assert -(-n // chunk) >= 3 and n % chunk == 7              # a short last chunk with a last wave of one pair


@pytest.mark.parametrize("route", list(CHUNKED))
def test_sweep_in_several_scratch_chunks(route):
    width, n = CHUNKED[route]
    case = _chunked_case()
    eng = _chunked_engine(width, capped=True)
    got = _run(eng, case["reads"][:n], case["refs"][:n])
    d = eng.describe(0, n)
    eng.close()
    assert d["ran_placed"] == route and -(-n // _chunk_pairs(width)) >= 3
    assert 0 < d["placed_scratch_bytes"] < case[route, "scratch"]              # the cap held: the rows of one chunk, not of the call
    _check(got, case[route], (route, "capped against uncapped"))
    _check(got[:16], case["ref16"], (route, "capped against the reference"))
    _check(case[route][:16], case["ref16"], (route, "uncapped against the reference"))


@pytest.mark.parametrize("route", list(CHUNKED))
def test_sweep_in_several_scratch_chunks_host_path(route):
    width, n = CHUNKED[route]
    case = _chunked_case()
    got = {}
    for capped in (True, False):
        eng = _chunked_engine(width, capped)
        got[capped] = _records(eng.score_placed_host(0, case["reads"][:n], case["refs"][:n], threads=2))
        d = eng.describe(0, n)
        assert d["ran_placed"] == route and -(-n // _chunk_pairs(width)) >= 3
        # (half a megabyte of sequence: the host call's direct small call -- the sweep's scratch chunks are what this checks, the
        # pipeline's slot loop is test_host_path_equals_device_path's)
        assert d["direct_call"] == 1
        eng.close()
    _check(got[True], got[False], (route, "host path, capped against uncapped"))
    _check(got[True], case[route], (route, "host path against device path"))
    _check(got[True][:16], case["ref16"], (route, "host path against the reference"))


def test_spanned_sweep_in_several_scratch_chunks():
    width, n = CHUNKED["strip"]
    case = _chunked_case()
    got = {}
    for capped in (True, False):
        eng = _chunked_engine(width, capped)
        got[capped] = _span(eng, case["reads"][:n], case["refs"][:n])
        assert eng.describe(0, n)["ran_span"].startswith("strip/") and -(-n // _chunk_pairs(width)) >= 3
        eng.close()
    _check(got[True], got[False], "spanned, capped against uncapped")
    _check(got[True][:, [0, 2, 4]], case["strip"], "spanned against placed records")


# ---- 10. seeded differential block ----
def _predict(R, F, sc, width, K):
    """placed_choice with the key on, unbanded, default tie-breaks (cell_rules.h), restated"""
    worst_gap = min(sc.gap_read, sc.gap_ref, sc.open_read, sc.open_ref, sc.ext_read, sc.ext_ref, 0)
    out_of_int16 = min(R, F) * max(sc.match, 0) + 1 > 32000 or min(sc.mismatch, 0) + worst_gap < -32000
    if width == 32 or out_of_int16:
        return "wide"
    if R > 1024:
        return "strip"
    bits = 2 if K <= 4 else (3 if K <= 8 else 4)
    return "key" if K <= 16 and ((min(R, F) * max(sc.match, 0) + 1) << bits) <= 32000 else "rows"


@pytest.mark.parametrize("block", range(4))
def test_seeded_differential(block):
    routes = set()
    for case in range(8 * block, 8 * block + 8):
        rng = np.random.default_rng(9000 + case)
        R = int(rng.integers(8, 1101)) if rng.random() < 0.6 else int(rng.choice([511, 512, 513, 1024, 1025]))
        F = int(rng.integers(8, 801)) if rng.random() < 0.6 else int(rng.choice([63, 64, 65, 128, 129]))
        n = int(rng.integers(1, 13))
        edge = 31999 // min(R, F)                          # the last match inside int16
        match = max(1, edge + int(rng.integers(-3, 4)))
        mismatch = -int(rng.integers(1, match + 1))
        gaps = [-int(rng.integers(1, 2 * match + 1)) for _ in range(6)]
        gaps[3], gaps[5] = -int(rng.integers(1, -gaps[2] + 1)), -int(rng.integers(1, -gaps[4] + 1))      # extending is not dearer than opening
        affine = bool(rng.integers(0, 2))
        sc = hipkernel.Scoring.make(match, mismatch, gaps[0], gaps[1], *(gaps[2:] if affine else []))
        width = int(rng.choice([0, 32]))
        reads, refs = _pairs(n, R, F, 9000 + case, indel_rate=float(rng.choice([0.0, 0.02])), sub_rate=float(rng.choice([0.02, 0.2])))
        eng = _engine(R, F, sc, width=width)
        got = _run(eng, reads, refs)
        d = eng.describe(0, n)
        eng.close()
        what = (case, R, F, n, match, mismatch, gaps, affine, width)
        assert d["ran_placed"] == _predict(R, F, sc, width, d["rows_per_lane"]), (what, d["ran_placed"])
        routes.add(d["ran_placed"])
        _check(got, placed_ref.placed(reads, refs, sc, affine=affine), what)
    assert "wide" in routes
