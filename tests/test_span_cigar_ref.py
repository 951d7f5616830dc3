"""The fact the spanned CIGARs rest on, checked on the CPU with tests/span_cigar_ref.py alone (numpy / plain Python): the
Default Smith-Waterman alignment of the two reversed prefixes that end in a pair's end cell

  * ends (its first walked cell) in the spanned record's begin cell,
  * walks to the reversed origin -- the forward end cell,
  * re-scored gives `score`, which is also the global score of the span (span_ref.global_scores),
  * and, read backwards, consumes exactly read_end - read_begin read bases and ref_end - ref_begin reference bases.

Every pair of every case is checked.  The inputs must exercise the claim: nearly every pair non-empty, gaps in every case."""
import numpy as np
import pytest

import span_cases as sc_
import span_cigar_ref
import span_ref

SHAPES = [(12, 20), (33, 70), (40, 9), (64, 128), (20, 120)]


@pytest.mark.parametrize("R,F", SHAPES)
def test_reversed_alignment_is_the_span(R, F):
    for form in sc_.FORMS:
        reads, refs, exp = span_cigar_ref.case(R, F, form)
        sc, affine = sc_.scoring(form), sc_.is_affine(form)
        spans, recs = exp["spans"], exp["recs"]
        glob = span_ref.global_scores(reads, refs, spans, sc, affine=affine)
        non_empty = gapped = 0
        for p in range(len(reads)):
            score, rb, re_, fb, fe = (int(v) for v in spans[p])
            walked = exp["walked"][p]
            if score == 0:
                assert not walked and not exp["ops"][p] and not recs[p].any(), (R, F, form, p, "empty")
                continue
            non_empty += 1
            first, last = walked[0], walked[-1]
            assert (re_ - 1 - first[0], fe - 1 - first[1]) == (rb, fb), (R, F, form, p, "ends in the spanned begin cell", first, spans[p].tolist())
            assert last == (0, 0), (R, F, form, p, "walk ends in the reversed origin", last)
            assert int(recs[p, 4]) == score == int(glob[p]), (R, F, form, p, "re-score", int(recs[p, 4]), score, int(glob[p]))
            assert span_cigar_ref.consumed(exp["ops"][p]) == (re_ - rb, fe - fb), (R, F, form, p, "bases consumed")
            assert tuple(recs[p, :4]) == (rb, re_, fb, fe) and int(recs[p, 5]) == len(exp["ops"][p]) > 0
            gapped += span_cigar_ref.has_gap(exp["ops"][p])
        assert non_empty >= 60, (R, F, form, non_empty)
        assert gapped >= 1, (R, F, form, gapped)
        if (R, F) in ((33, 70), (64, 128)):
            assert gapped >= 20, (R, F, form, gapped)


def test_ops_are_in_forward_reading_order():
    """the rows put back in forward order are the span's own bases: degapped, read[read_begin:read_end] and ref[ref_begin:ref_end]"""
    R, F = 33, 70
    for form in ("lin", "aff"):
        reads, refs, exp = span_cigar_ref.case(R, F, form)
        for p in range(len(reads)):
            score, rb, re_, fb, fe = (int(v) for v in exp["spans"][p])
            s, e = int(exp["idx"][p, 0]), int(exp["idx"][p, 1])
            a, b = exp["rows"][p, 0, s:e], exp["rows"][p, 1, s:e]
            if score == 0:
                continue
            assert a[a != span_cigar_ref.GAP].tobytes() == reads[p, rb:re_].tobytes(), (form, p)
            assert b[b != span_cigar_ref.GAP].tobytes() == refs[p, fb:fe].tobytes(), (form, p)


def test_clip_changes_nothing():
    """20 x 120: span_ref_length is 33 - 59 columns; the alignment of the CLIPPED reversed prefixes is the unclipped one"""
    R, F = 20, 120
    for form in sc_.FORMS:
        reads, refs, exp = span_cigar_ref.case(R, F, form)
        sc, affine = sc_.scoring(form), sc_.is_affine(form)
        Fr = sc_.span_ref_length(R, F, sc)
        assert 33 <= Fr <= 59
        rr = span_ref._reversed_prefixes(reads, exp["spans"][:, 2])
        rf = span_ref._reversed_prefixes(refs, exp["spans"][:, 4])[:, :Fr]
        _, _, walked = span_cigar_ref.band_align_ref.align_banded_sw(rr, np.ascontiguousarray(rf), 2 * F + 2, sc, affine=affine, paths=True)
        assert walked == exp["walked"], form
        assert (exp["spans"][:, 4] > Fr).any(), "no prefix is longer than the clip"
