"""tests/span_ref.py -- the numpy restatement the GPU tests of the spanned scores compare against -- pinned on the CPU: the
reverse maximum is the forward score, the span's global alignment score is the score, the end is the placed record's, clipping
the reversed reference to span_ref_length columns changes nothing, and hand-built ties begin where the construction says."""
import functools

import numpy as np
import pytest

import placed_ref
import span_cases as sc_
import span_ref
from versalignlib_amd import hipkernel


@functools.lru_cache(maxsize=None)
def _case(R, F, form, indel=False):
    if indel:
        reads, refs = sc_.pairs(64, R, F, 31 * R + F, indel_rate=0.15)
        sc = hipkernel.Scoring.make(3, -1, -1, -1) if form == "sym" else hipkernel.Scoring.make(3, -1, -1, -1, -1, -1, -1, -1)
    else:
        reads, refs = sc_.pairs(64, R, F, 11 * R + F)
        sc = sc_.scoring(form)
    recs, rev_max = span_ref.spans(reads, refs, sc, affine=sc_.is_affine(form), with_reverse_max=True)
    return reads, refs, sc, recs, rev_max


@pytest.mark.parametrize("form", list(sc_.FORMS))
@pytest.mark.parametrize("R,F", sc_.SHAPES)
def test_definition_holds(R, F, form):
    reads, refs, sc, recs, rev_max = _case(R, F, form)
    affine = sc_.is_affine(form)
    pl = placed_ref.placed(reads, refs, sc, affine=affine)
    assert np.array_equal(recs[:, [0, 2, 4]], pl)                                     # score and end: the placed record
    assert np.array_equal(rev_max, pl[:, 0])                                          # the reverse maximum is the forward score
    assert (recs[:, 0] > 0).sum() >= 32
    assert (recs[:, 1] <= recs[:, 2]).all() and (recs[:, 3] <= recs[:, 4]).all() and (recs >= 0).all()
    hit = recs[:, 0] > 0
    assert (recs[hit, 1] < recs[hit, 2]).all() and (recs[hit, 3] < recs[hit, 4]).all()
    assert np.array_equal(span_ref.global_scores(reads, refs, recs, sc, affine=affine), recs[:, 0])
    Fr = sc_.span_ref_length(R, F, sc)
    assert np.array_equal(span_ref.spans(reads, refs, sc, affine=affine, clip=Fr), recs), ("clipped to", Fr)


@pytest.mark.parametrize("form", ["sym", "affsym"])
@pytest.mark.parametrize("R,F", sc_.SHAPES)
def test_indel_heavy_pairs_under_cheap_gaps(R, F, form):
    reads, refs, sc, recs, rev_max = _case(R, F, form, indel=True)
    affine = sc_.is_affine(form)
    assert np.array_equal(rev_max, recs[:, 0])
    assert np.array_equal(span_ref.global_scores(reads, refs, recs, sc, affine=affine), recs[:, 0])
    Fr = sc_.span_ref_length(R, F, sc)
    assert Fr == min(F, R + (3 * R - 1))
    assert np.array_equal(span_ref.spans(reads, refs, sc, affine=affine, clip=Fr), recs)
    # the spans do hold gaps: some cover more reference columns than read rows, some fewer
    width = (recs[:, 4] - recs[:, 3]) - (recs[:, 2] - recs[:, 1])
    assert (width > 0).any() and (width < 0).any() or min(R, F) < 12


def test_worked_values_of_the_bound():
    assert sc_.span_ref_length(20, 120, hipkernel.Scoring.make(2, -1, -3, -3)) == 33
    assert sc_.span_ref_length(150, 500, hipkernel.Scoring.make(2, -1, -3, -3)) == 249
    assert sc_.span_ref_length(150, 500, hipkernel.Scoring.make(2, -1, -3, -3, -5, -1, -5, -1)) == 449


@pytest.mark.parametrize("form", ["sym", "aff"])
@pytest.mark.parametrize("R,F", [(33, 70), (40, 9), (150, 200)])
def test_hand_built_ties_begin_at_the_later_cell(R, F, form):
    sc = sc_.tie_scoring(form)
    for name, (reads, refs, exp) in sc_.tie_batches(R, F).items():
        got = span_ref.spans(reads, refs, sc, affine=form == "aff")
        assert np.array_equal(got, exp), (name, got[:4].tolist(), exp[:4].tolist())
        if name == "zero_block":
            # ... and the earlier begin is a true tie: the span that takes the zero block in scores the same globally
            wider = exp.copy()
            wider[:, 1] -= 2
            wider[:, 3] -= 2
            assert np.array_equal(span_ref.global_scores(reads, refs, wider, sc, affine=form == "aff"), exp[:, 0])


@pytest.mark.parametrize("R,F", [(12, 20), (40, 9), (20, 120)])
def test_borders(R, F):
    reads, refs, exp = sc_.border_batch(R, F)
    for form in ("sym", "aff"):
        got = span_ref.spans(reads, refs, sc_.scoring(form), affine=sc_.is_affine(form))
        assert np.array_equal(got, exp), (form, got.tolist(), exp.tolist())


def test_all_n_pairs_are_five_zeros():
    reads, refs = sc_.pairs(16, 30, 50, 5)
    reads[::2] = ord("N")
    for form in ("sym", "aff"):
        got = span_ref.spans(reads, refs, sc_.scoring(form), affine=sc_.is_affine(form))
        assert not got[::2].any() and got[1::2, 0].all()
