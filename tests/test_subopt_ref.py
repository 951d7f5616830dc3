"""tests/subopt_ref.py -- the numpy restatement the GPU tests of the suboptimal scores compare against -- pinned on the CPU
against hand-worked cases: the runner-up of a planted second copy, the padded-read case that shows why rows beyond the trimmed
length are no candidates, the empty window, score2 <= score, and ties that go to the smaller column."""
import numpy as np
import pytest

import placed_ref
import subopt_cases as cases
import subopt_ref
from versalignlib_amd import hipkernel

LIN = hipkernel.Scoring.make(2, -1, -3, -3)
AFF = hipkernel.Scoring.make(2, -1, -3, -3, -3, -3, -3, -3)


def _two_copies():
    # a reference of one repeated base the read's neighbourhood cannot extend into: T runs, the read drawn from ACG only
    rd = np.frombuffer(b"ACGACCGAGCAGGCACGAGCCAGC", np.uint8).copy()
    ref = np.full(140, ord("T"), np.uint8)
    ref[20:44] = rd
    ref[90:114] = cases.mutate(rd, [6, 12, 18])
    return rd[None, :], ref[None, :]


@pytest.mark.parametrize("sc,affine", [(LIN, False), (AFF, True)])
def test_second_copy_with_three_mismatches(sc, affine):
    reads, refs = _two_copies()
    got = subopt_ref.subopt(reads, refs, sc, 12, affine=affine)
    assert got.tolist() == [[48, 24, 44, 39, 114]]


def test_padded_reads_trimmed_and_untrimmed():
    R, F, mask = 40, 120, 15
    best, all_rows, trimmed = [], [], []
    for L in (30, 20, 12):
        reads, refs = cases.planted(1, R, F, seed=100 + L, read_len=L, at=50, pad=0)
        t = subopt_ref.subopt(reads, refs, LIN, mask)
        u = subopt_ref.subopt(reads, refs, LIN, mask, trim=False)
        assert np.array_equal(t[:, :3], u[:, :3])
        best.append(int(t[0, 0]))
        trimmed.append(int(t[0, 3]))
        all_rows.append(int(u[0, 3]))
    assert best == [60, 40, 24]
    # through the padding the best score runs down its diagonal and leaves the window: the untrimmed runner-up repeats it
    assert all_rows[1] == 40 and all_rows[2] == 24 and all_rows[0] > trimmed[0]
    assert all(t < b for t, b in zip(trimmed, best))


def test_mask_at_least_F_leaves_no_candidate():
    reads, refs = cases.planted(8, 33, 70, seed=3, at=10)
    for mask in (70, 71, 10 ** 6):
        got = subopt_ref.subopt(reads, refs, LIN, mask)
        assert (got[:, 0] > 0).all() and (got[:, 3:] == 0).all()
    assert (subopt_ref.subopt(reads, refs, LIN, 69)[:, 3:] == 0).all()          # |j - c| <= 69 for every column of 70


@pytest.mark.parametrize("mask", [0, 5, 16, 40])
def test_score2_never_exceeds_score(mask):
    reads, refs, _ = cases.fuzz_batch(64, 33, 70, seed=mask)
    for sc, affine in ((LIN, False), (AFF, True)):
        got = subopt_ref.subopt(reads, refs, sc, mask, affine=affine)
        assert (got[:, 3] <= got[:, 0]).all() and (got >= 0).all()
        assert np.array_equal(got[:, :3], placed_ref.placed(reads, refs, sc, affine=affine))
        hit = got[:, 3] > 0
        assert (np.abs(got[hit, 4] - got[hit, 2]) > mask).all()
        assert ((got[:, 3] == 0) == (got[:, 4] == 0)).all()


def test_ties_go_to_the_smaller_column():
    # the best copy (8 bases) in the middle, two equal shorter copies (5 bases) left and right of the window
    rd = np.frombuffer(b"ACGACCGA", np.uint8)
    ref = np.full(80, ord("T"), np.uint8)
    ref[40:48] = rd
    ref[10:15] = rd[:5]
    ref[65:70] = rd[:5]
    got = subopt_ref.subopt(rd[None, :], ref[None, :], LIN, 6)
    assert got.tolist() == [[16, 8, 48, 10, 15]]
    # two exact copies: the first one is the placed record, the runner-up equals the score at the later column
    ref = np.full(80, ord("T"), np.uint8)
    ref[10:18] = rd
    ref[50:58] = rd
    got = subopt_ref.subopt(rd[None, :], ref[None, :], LIN, 6)
    assert got.tolist() == [[16, 8, 18, 16, 58]]


def test_trimmed_lengths():
    s = np.frombuffer(b"ACGTNN\0\0" b"NNNNNNNN" b"acgNtNNa" b"\0\0\0\0\0\0\0G", np.uint8).reshape(4, 8)
    assert subopt_ref.trimmed_lengths(s).tolist() == [4, 0, 8, 8]
    # columns at or beyond the trimmed reference length are no candidates
    rd = np.frombuffer(b"ACGACCGA", np.uint8)
    ref = np.zeros(60, np.uint8)
    ref[5:13] = rd
    ref[30:35] = rd[:5]
    got = subopt_ref.subopt(rd[None, :], ref[None, :], LIN, 6)
    assert got.tolist() == [[16, 8, 13, 10, 35]]
    ref[33:] = ord("N")                              # Fp = 33: the second copy is cut to three bases
    assert subopt_ref.subopt(rd[None, :], ref[None, :], LIN, 6).tolist() == [[16, 8, 13, 6, 33]]
