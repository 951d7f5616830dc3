"""tests/placed_band_ref.py (the numpy statement of banded placed scores) against what already stands: its scores are the
oracle's banded Smith-Waterman scores on the chain's block band, a band wider than the matrix gives tests/placed_ref.py's
unbanded records, and a band does change the record where the better motif lies outside it.  No GPU."""
import numpy as np
import pytest

import placed_band_ref
import placed_ref
from band_align_ref import row_window
from oracle import cpu_ref
from versalignlib_amd import synth

FORMS = {"sym": (-3, -3), "lin": (-2, -4), "affsym": (-3, -3, -5, -1, -5, -1), "aff": (-3, -3, -6, -2, -4, -1)}
SHAPES = [(31, 33, 6), (100, 120, 8), (513, 400, 24), (300, 700, 2), (200, 90, 40)]


def _pairs(n, R, F, seed):
    return synth.make_pairs(n, R, F, seed=seed, sub_rate=0.1, indel_rate=0.02, n_run_frac=0.1, short_frac=0.1, lowercase_frac=0.05, junk_frac=0.04)


@pytest.mark.parametrize("form", list(FORMS))
def test_scores_are_the_oracles_block_band(form):
    sc = cpu_ref.Scoring.make(2, -1, *FORMS[form])
    affine = len(FORMS[form]) > 2
    for R, F, band in SHAPES:
        reads, refs = _pairs(12, R, F, R + F + band)
        got = placed_band_ref.placed_banded(reads, refs, band, sc, affine=affine)
        exp = cpu_ref.score_banded_sw(reads, refs, band, sc, threads=2, block_rows=16, col_align=1, affine=affine)
        assert np.array_equal(got[:, 0], exp.astype(np.int64)), (form, R, F, band, got[:, 0], exp)
        # every end cell lies inside its row's window, and empty records are all zero
        for p in range(len(got)):
            s, i, j = got[p]
            if s == 0:
                assert i == 0 and j == 0
            else:
                lo, hi = row_window(i - 1, R, F, band, 16, 1)
                assert lo <= j - 1 <= hi, (form, R, F, band, p, got[p], lo, hi)
        assert (got[:, 0] > 0).any()


@pytest.mark.parametrize("form", list(FORMS))
def test_a_band_wider_than_the_matrix_is_the_unbanded_record(form):
    sc = cpu_ref.Scoring.make(2, -1, *FORMS[form])
    affine = len(FORMS[form]) > 2
    for R, F in [(31, 33), (100, 120), (130, 70), (257, 300)]:
        reads, refs = _pairs(10, R, F, 7 * R + F)
        got = placed_band_ref.placed_banded(reads, refs, 2 * max(R, F), sc, affine=affine)
        exp = placed_ref.placed(reads, refs, sc, affine=affine)
        assert np.array_equal(got, exp), (form, R, F, got, exp)


def test_the_band_changes_the_record_where_the_better_motif_lies_outside_it():
    R, F, band = 200, 200, 16
    reads = np.full((2, R), ord("N"), np.uint8)
    refs = np.full((2, F), ord("N"), np.uint8)
    long_motif = np.frombuffer(b"ACGTTGCAAGGCTTACGATC", np.uint8)      # 20 bases, far off the diagonal
    short_motif = np.frombuffer(b"GATTACAGGT", np.uint8)               # 10 bases, on it
    for p in range(2):
        reads[p, 20:40] = long_motif
        refs[p, 150:170] = long_motif                                 # column - row = 130: outside a band of 16
        reads[p, 100:110] = short_motif
        refs[p, 100 + 3 * p:110 + 3 * p] = short_motif
    sc = cpu_ref.Scoring.make(2, -5, -5, -5)
    assert row_window(39, R, F, band, 16, 1)[1] < 150
    banded = placed_band_ref.placed_banded(reads, refs, band, sc)
    full = placed_ref.placed(reads, refs, sc)
    assert full.tolist() == [[40, 40, 170], [40, 40, 170]]
    assert banded.tolist() == [[20, 110, 110], [20, 110, 113]]
    aff = cpu_ref.Scoring.make(2, -5, -5, -5, -7, -5, -7, -5)
    assert placed_band_ref.placed_banded(reads, refs, band, aff, affine=True).tolist() == banded.tolist()
