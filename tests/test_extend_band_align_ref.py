"""tests/extend_band_align_ref.py against what it must agree with, on the CPU: its extension records are extend_band_ref's; with
w >= max(R, F) its results are extend_align_ref's; every walked cell is present; the ops re-score to X(end cell); an unreached read
end is never chosen at end_bonus = INT32_MAX; and a B = 1 example worked out by hand."""
import numpy as np
import pytest

import extend_align_ref as ear
import extend_band_align_ref as ref
import extend_band_ref as ebr
from versalignlib_amd import hipkernel

FORMS = {"sym": (-3, -3), "lin": (-2, -4), "affsym": (-3, -3, -5, -1, -5, -1), "aff": (-3, -3, -6, -2, -4, -1)}
BASES = np.frombuffer(b"ACGT", np.uint8)
BONUSES = (-1, ref.INT32_MAX, 20)


def _scoring(form, match=2, mismatch=-1):
    return hipkernel.Scoring.make(match, mismatch, *FORMS[form])


def _pairs(n, R, F, seed):
    """reads against references that share a prefix, some with extra reference bases, some trimmed, one reference cut short"""
    rng = np.random.default_rng(seed)
    reads, refs = BASES[rng.integers(0, 4, (n, R))], BASES[rng.integers(0, 4, (n, F))]
    for p in range(n):
        L = int(rng.integers(1, min(R, F) + 1))
        d = int(rng.integers(0, 6)) if p % 2 else 0
        refs[p, d:d + min(L, F - d)] = reads[p, :min(L, F - d)]
        if p % 3 == 0:
            reads[p, int(rng.integers(1, R + 1)):] = ord("N")
        if p % 4 == 1:
            refs[p, int(rng.integers(1, F + 1)):] = 0
    refs[n - 1, 3:] = 0
    return reads, refs


@pytest.mark.parametrize("band_width", [1, 2, 9, 17, 40])
@pytest.mark.parametrize("form", list(FORMS))
def test_records_paths_and_scores(form, band_width):
    R, F = 33, 41
    reads, refs = _pairs(12, R, F, seed=band_width)
    sc, affine = _scoring(form), len(FORMS[form]) > 2
    results = ref.align(reads, refs, sc, band_width, affine, end_bonus=BONUSES, extended=True)
    records = ebr.extend(reads, refs, sc, band_width, affine=affine)
    P = ebr.present(R, F, band_width)
    Rp = ref.trimmed_lengths(reads)
    X, _, _, _, _ = ref.matrices(reads, refs, sc, band_width, affine)
    for bonus, (recs, ops, ext, ends, paths) in zip(BONUSES, results):
        assert np.array_equal(ext, records), (form, band_width, bonus)
        assert any(e is not None for e in ends)
        for p, (cell, moves) in enumerate(zip(ends, paths)):
            if cell is None:
                assert recs[p].tolist() == [0] * 6 and ops[p] == []
                continue
            assert all(P[i + 1, j + 1] for _, i, j in moves), (form, band_width, p, "the walk left the band")
            assert recs[p, 4] == X[p, cell[0] + 1, cell[1] + 1]                          # re-score == X(end cell)
            assert sum(k != "D" for k, _, _ in moves) == recs[p, 1] and sum(k != "I" for k, _, _ in moves) == recs[p, 3]
            assert sum(op >> 4 for op in ops[p]) == len(moves)
            if ext[p, 3] == ebr.UNREACHED:
                assert cell[0] != Rp[p] - 1 or cell == (int(ext[p, 1]) - 1, int(ext[p, 2]) - 1), (p, cell, "an unreached read end was chosen")
    # an unreached read end exists in the narrow bands, and INT32_MAX picks the read end wherever it is reached
    always = results[1]
    if band_width <= 17:
        assert (always[2][:, 3] == ebr.UNREACHED).any()
    for p, cell in enumerate(always[3]):
        if Rp[p] > 0 and always[2][p, 3] != ebr.UNREACHED:
            assert cell == (Rp[p] - 1, always[2][p, 4] - 1)
        elif Rp[p] > 0:
            assert cell is None or cell == (always[2][p, 1] - 1, always[2][p, 2] - 1)


@pytest.mark.parametrize("form", list(FORMS))
def test_the_limit_is_the_unbanded_alignment(form):
    R, F = 19, 27
    reads, refs = _pairs(10, R, F, seed=5)
    sc, affine = _scoring(form), len(FORMS[form]) > 2
    for band_width in (2 * F, 2 * F + 1, 400):
        got = ref.align(reads, refs, sc, band_width, affine, end_bonus=BONUSES)
        want = ear.align(reads, refs, sc, affine, end_bonus=BONUSES)
        for g, w in zip(got, want):
            assert np.array_equal(g[0], w[0]) and g[1] == w[1] and np.array_equal(g[2], w[2]) and g[3] == w[3]
    narrow = ref.align(reads, refs, sc, 3, affine, end_bonus=-1)
    assert not np.array_equal(narrow[0], want[0][0])                # (a band that matters changes something)


def test_hand_checked_per_cell_band():
    """B = 1, band_width 2 (w = 1): |i - j| <= 1.  read ACGT, ref AGT + padding, match 2, mismatch -1, gaps -3 (linear).
    Present cells row by row (X):            j = -1    0    1    2
        i = -1                                    0   -3    .    .
        i = 0  (A)                               -3    2   -1    .
        i = 1  (C)                                .   -1    1   -2
        i = 2  (G)                                .    .    1    0
        i = 3  (T)                                .    .    .    3
    X(1,1) = max(2 + S(C,G) = 1, X(1,0) - 3, X(0,1) - 3) = 1;  X(2,1) = max(X(1,0) + S(G,G) = 1, X(1,1) - 3) = 1;
    X(2,2) = max(X(1,1) + S(G,T) = 0, X(2,1) - 3 = -2, X(1,2) - 3 = -5) = 0;  X(3,2) = max(X(2,1) + S(T,T) = 3, X(2,2) - 3) = 3.
    The best cell is (3, 2) with 3, which is also the read end: A = | C I | G = | T =  ->  1=, 1I, 2=."""
    sc = hipkernel.Scoring.make(2, -1, -3, -3)
    reads = np.frombuffer(b"ACGT", np.uint8)[None, :]
    refs = np.frombuffer(b"AGT\0", np.uint8)[None, :].copy()
    X, _, _, _, P = ref.matrices(reads, refs, sc, 2, False, B=1)
    rows = [[int(X[0, i, j]) if P[i, j] else None for j in range(4)] for i in range(5)]
    assert rows == [[0, -3, None, None], [-3, 2, -1, None], [None, -1, 1, -2], [None, None, 1, 0], [None, None, None, 3]]
    for bonus in BONUSES:
        recs, ops, ext, ends, paths = ref.align(reads, refs, sc, 2, False, end_bonus=bonus, extended=True, B=1)
        assert ext[0].tolist() == [3, 4, 3, 3, 3] and ends == [(3, 2)]
        assert recs[0].tolist() == [0, 4, 0, 3, 3, 3]
        assert ops[0] == [(1 << 4) | ear.OP_EQ, (1 << 4) | ear.OP_I, (2 << 4) | ear.OP_EQ]
        assert [k for k, _, _ in paths[0]] == ["M", "I", "M", "M"]
    # one base more of band (w = 0 -> only the diagonal and, B = 1, nothing else): the read end is reached through mismatches
    recs, ops, ext, ends, _ = ref.align(reads, refs, sc, 1, False, end_bonus=ref.INT32_MAX, B=1)
    assert ext[0].tolist() == [2, 1, 1, ebr.UNREACHED, 0] and ends == [(0, 0)] and recs[0].tolist() == [0, 1, 0, 1, 2, 1]
