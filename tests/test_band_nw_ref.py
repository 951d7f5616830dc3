"""The numpy restatement of the banded NW variant (band_nw_ref.py) pinned to the reference-pinned oracle: a band of at least
2 * max(R, F) is the unbanded oracle (scores and alignments, linear and affine gaps, reads with short tails and N runs), scores
obey per-cell band <= block band <= unbanded, an absent start cell gives the empty alignment, and bands whose windows do not
connect are refused."""
import numpy as np
import pytest

from oracle import cpu_ref
from versalignlib_amd import synth
import band_nw_ref as bnr
from band_align_ref import row_window
from test_band_align_ref import shifted_insertion_pairs

LINEAR = cpu_ref.Scoring.make(2, -1, -3, -2)
AFFINE = cpu_ref.Scoring.make(2, -1, -3, -3, -5, -1, -4, -2)
BLOCKS = [(1, 1), (16, 1), (160, 4)]


def _pairs(n, R, F, seed):
    return synth.make_pairs(n, R, F, seed=seed, sub_rate=0.1, indel_rate=0.01, n_run_frac=0.2, short_frac=0.15,
                            lowercase_frac=0.05, junk_frac=0.05)


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("R,F,seed", [(150, 500, 1), (300, 260, 2), (97, 97, 3)])
def test_wide_band_is_the_unbanded_oracle(affine, R, F, seed):
    reads, refs = _pairs(40, R, F, seed)
    sc = AFFINE if affine else LINEAR
    exp_scores = cpu_ref.score(1, reads, refs, sc, threads=4, affine=affine)
    exp_rows, exp_idx = cpu_ref.align(1, reads, refs, sc, threads=4, affine=affine)
    for block_rows, col_align in BLOCKS:
        scores = bnr.score_banded_nw(reads, refs, 2 * max(R, F), sc, block_rows, col_align, affine=affine)
        assert np.array_equal(scores, exp_scores.astype(np.int64)), (block_rows, col_align)
        rows, idx = bnr.align_banded_nw(reads, refs, 2 * max(R, F), sc, block_rows, col_align, affine=affine)
        assert np.array_equal(idx, exp_idx) and np.array_equal(rows, exp_rows), (block_rows, col_align)


@pytest.mark.parametrize("affine", [False, True])
def test_score_sandwich_and_a_batch_where_the_three_differ(affine):
    reads, refs = shifted_insertion_pairs(n=16)
    sc = AFFINE if affine else LINEAR
    unbanded = cpu_ref.score(1, reads, refs, sc, threads=4, affine=affine).astype(np.int64)
    cell = bnr.score_banded_nw(reads, refs, 64, sc, 1, 1, affine=affine)
    chain = bnr.score_banded_nw(reads, refs, 64, sc, 16, 1, affine=affine)
    strips = bnr.score_banded_nw(reads, refs, 64, sc, 160, 4, affine=affine)
    assert (cell <= chain).all() and (chain <= strips).all() and (strips <= unbanded).all()
    assert (cell < chain).any() and (chain < strips).any() and (strips < unbanded).any()
    reads, refs = _pairs(24, 320, 410, 5)
    unbanded = cpu_ref.score(1, reads, refs, sc, threads=4, affine=affine).astype(np.int64)
    for band in (2, 16, 64, 300):
        cell = bnr.score_banded_nw(reads, refs, band, sc, 1, 1, affine=affine)
        for block_rows, col_align in BLOCKS[1:]:
            block = bnr.score_banded_nw(reads, refs, band, sc, block_rows, col_align, affine=affine)
            assert (cell <= block).all() and (block <= unbanded).all(), (band, block_rows)


@pytest.mark.parametrize("affine", [False, True])
def test_banded_alignments_stay_in_the_band_and_end_where_the_rule_says(affine):
    """The walk asserts that no pointer leaves the band; the alignment consumes the read up to its first invalid byte."""
    R, F = 320, 410
    reads, refs = _pairs(30, R, F, 7)
    sc = AFFINE if affine else LINEAR
    for band in (2, 16, 64):
        for block_rows, col_align in BLOCKS:
            rows, idx = bnr.align_banded_nw(reads, refs, band, sc, block_rows, col_align, affine=affine)
            for p in range(len(reads)):
                s, e = int(idx[p, 0]), int(idx[p, 1])
                read_row = rows[p, 0, s:e]
                consumed = bytes(read_row[read_row != ord("-")])
                assert bytes(reads[p]).startswith(consumed)


@pytest.mark.parametrize("affine", [False, True])
def test_absent_start_cell_is_the_empty_alignment(affine):
    """The reference's first byte is invalid (last_ref = -1) while the last read row's window starts beyond column 0."""
    R, F, band = 200, 200, 16
    reads, refs = synth.make_pairs(4, R, F, seed=9, sub_rate=0.05)
    refs[1, 0] = 0
    refs[2, 40] = 0                                  # last_ref = 39 < lo of row R - 1
    assert row_window(R - 1, R, F, band, 16, 1)[0] > 40
    sc = AFFINE if affine else LINEAR
    rows, idx = bnr.align_banded_nw(reads, refs, band, sc, 16, 1, affine=affine)
    for p in (1, 2):
        assert not rows[p].any() and (idx[p] == R + F - 1).all()
    for p in (0, 3):
        assert rows[p].any() and idx[p, 0] < R + F - 1


def test_windows_that_do_not_connect_are_refused():
    reads, refs = synth.make_pairs(2, 100, 1000, seed=10)
    for fn in (bnr.score_banded_nw, bnr.align_banded_nw):
        with pytest.raises(ValueError, match="do not connect"):
            fn(reads, refs, 8, LINEAR)               # 2 * 4 + 1 = 9 < ceil(1000 / 100) = 10
        fn(reads, refs, 10, LINEAR)                  # 11 >= 10
