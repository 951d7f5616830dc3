"""tests/extend_zdrop_ref.py against itself, on the CPU: Z = 2^29 is the record without the key (tests/extend_ref.py unbanded,
tests/extend_band_ref.py under a band); the drop row never moves up as Z grows; the record is the brute-force row-major first
maximum over the rows before T; a 6 x 8 case worked out by hand; the count of skipped waves on drop rows written down."""
import numpy as np
import pytest

import extend_band_ref as ebr
import extend_ref
import extend_zdrop_ref as ezr
from versalignlib_amd import hipkernel

BASES = np.frombuffer(b"ACGT", np.uint8)
FORMS = {"lin": (-4, -4), "lin2": (-2, -4), "aff": (-5, -1, -6, -2)}


def _scoring(form):
    return hipkernel.Scoring.make(2, -3, *FORMS[form])


def _planted(n, R, F, seed):
    """pair k: the reference is the read's first a_k bases, then g_k bases of C against a read of A, then the read again"""
    rng = np.random.default_rng(seed)
    reads = BASES[rng.integers(0, 4, (n, R))]
    refs = BASES[rng.integers(0, 4, (n, F))]
    for k in range(n):
        a, g = int(rng.integers(5, R // 2)), int(rng.integers(4, 12))
        reads[k, a:a + g] = ord("A")
        refs[k, :a] = reads[k, :a]
        refs[k, a:a + g] = ord("C")
        tail = min(R, F) - a - g
        refs[k, a + g:a + g + tail] = reads[k, a + g:a + g + tail]
    reads[1, R - 7:] = ord("N")
    refs[2, F - 9:] = 0
    return reads, refs


@pytest.mark.parametrize("band_width", [0, 9, 40])
@pytest.mark.parametrize("form", list(FORMS))
def test_never_dropping_is_the_record_without_the_key(form, band_width):
    reads, refs = _planted(6, 40, 52, seed=3)
    sc, affine = _scoring(form), len(FORMS[form]) > 2
    got, T = ezr.extend(reads, refs, sc, ezr.NEVER_DROPS, band_width, affine)
    exp = ebr.extend(reads, refs, sc, band_width, affine) if band_width else extend_ref.extend(reads, refs, sc, affine)
    assert np.array_equal(got, exp) and np.array_equal(T, extend_ref.trimmed_lengths(reads))


@pytest.mark.parametrize("band_width", [0, 16])
@pytest.mark.parametrize("form", list(FORMS))
def test_drop_rows_grow_with_Z_and_the_record_is_the_best_cell_before_T(form, band_width):
    R, F = 40, 52
    reads, refs = _planted(6, R, F, seed=5)
    sc, affine = _scoring(form), len(FORMS[form]) > 2
    X, P = ebr.matrices(reads, refs, sc, band_width if band_width else 2 * max(R, F) + 2, affine)
    Rp, Fp = extend_ref.trimmed_lengths(reads), extend_ref.trimmed_lengths(refs)
    last, dropped = None, 0
    for Z in (1, 5, 10, 30, 100, 1 << 29):
        got, T = ezr.extend(reads, refs, sc, Z, band_width, affine)
        assert last is None or (T >= last).all(), Z
        last = T
        dropped += int((T < Rp).sum())
        for k in range(len(reads)):
            best, bi, bj = 0, 0, 0
            for i in range(int(T[k])):
                for j in range(int(Fp[k])):
                    if P[i + 1, j + 1] and X[k, i + 1, j + 1] > best:
                        best, bi, bj = int(X[k, i + 1, j + 1]), i + 1, j + 1
            assert got[k, :3].tolist() == [best, bi, bj], (Z, k)
            if T[k] < Rp[k]:
                assert got[k, 3:].tolist() == [ezr.UNREACHED, 0], (Z, k)
    assert dropped > 0 and (last == Rp).all()


def test_a_case_worked_out_by_hand():
    """read ACGGGG, reference ACTTTTTT, match 2 / mismatch -3 / gaps -4.  Rows 0 and 1 match on the diagonal: m = 2, 4 at columns
    0, 1.  From row 2 on the best cell of a row is the diagonal one -- X(2, 2) = 4 - 3 = 1, X(3, 3) = -2, X(4, 4) = -5, X(5, 5) = -8
    (a gap costs 4, more than a mismatch) -- so di = dj, the penalty is 0 and row i drops iff 4 - m_i > Z: row 2 for Z < 3, row 3
    for Z < 6, row 4 for Z < 9, row 5 for Z < 12."""
    reads = np.frombuffer(b"ACGGGG", np.uint8)[None, :]
    refs = np.frombuffer(b"ACTTTTTT", np.uint8)[None, :]
    sc = hipkernel.Scoring.make(2, -3, -4, -4)
    X, P = ebr.matrices(reads, refs, sc, 30)
    assert ezr.row_maxima(X[0], P, 6, 8) == [(0, 2, 0), (1, 4, 1), (2, 1, 2), (3, -2, 3), (4, -5, 4), (5, -8, 5)]
    for Z, T in ((1, 2), (2, 2), (3, 3), (5, 3), (6, 4), (8, 4), (9, 5), (11, 5), (12, 6), (1 << 29, 6)):
        got, drop_row = ezr.extend(reads, refs, sc, Z)
        assert drop_row.tolist() == [T], (Z, drop_row)
        assert got[0].tolist() == ([4, 2, 2, ezr.UNREACHED, 0] if T < 6 else [4, 2, 2, -8, 6]), (Z, got)
    # an offset diagonal is paid for: the same rows with the row's maximum one column further right
    best = ((4, 1, 1), 2)
    assert ezr.drop([(0, 2, 0), (1, 4, 1), (2, 1, 3)], 6, 2, 4, 4) == ((4, 1, 1), 6)        # 4 - 1 - 1 * 4 = -1: no drop
    assert ezr.drop([(0, 2, 0), (1, 4, 1), (2, 1, 2)], 6, 2, 4, 4) == best                  # 4 - 1 - 0 = 3 > 2
    assert ezr.drop([(0, 2, 0), (1, 4, 1), (3, 1, 2)], 6, 2, 0, 4) == ((4, 1, 1), 3)        # di > dj at price 0


def test_skipped_waves_on_written_down_drop_rows():
    # R = 1030: strips at rows 512 and 1024.  Waves (0, 1), (2, 3), (4)
    Rp = [1030, 1030, 1030, 600, 1030]
    Fp = [1100] * 5
    none = lambda k: Rp[k]
    assert ezr.skipped_waves([100, 511, 100, none(3), 100], Rp, Fp, 1030, 0) == 2 + 0 + 2
    assert ezr.skipped_waves([100, 512, 100, 100, 1023], Rp, Fp, 1030, 0) == 1 + 2 + 1            # T = 512: strip 1 runs
    assert ezr.skipped_waves([none(0)] * 5, Rp, Fp, 1030, 0) == 0
    # Rp = 600 twice: strip 2 would not have run, so it is not counted as skipped
    assert ezr.skipped_waves([100, 100], [600, 600], [700, 700], 1030, 0) == 1
    # under a band: a strip whose window holds no column below the larger Fp returns as empty, before the skip is looked at
    assert ezr.skipped_waves([100, 100], [1030, 1030], [400, 300], 1030, 32) == 0
    assert ezr.skipped_waves([100, 100], [1030, 1030], [400, 600], 1030, 32) == 1                 # strip 1's window starts at 496
