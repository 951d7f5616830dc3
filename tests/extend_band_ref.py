"""Banded extension scores (include/valign_hip.h: valign_hip_set_extend_band) restated in numpy, independent of the library: the
whole matrix of tests/extend_ref.py on int64 cells, with the cells outside the band ABSENT -- a value no maximum takes.

  band: w = band_width // 2; rows in blocks of B consecutive read positions counted from row 0 (the library: B = 8; B = 1 is the
  per-cell band |i - j| <= w).  Cell (i, j), 0 <= i < R, -1 <= j < F, is present iff B * (i // B) - w <= j <= B * (i // B) + B - 1
  + w; cell (-1, j) iff j + 1 <= w.  An absent cell is no candidate of a neighbour, a maximum or an arg-max; with affine gaps all
  three of its states are absent.  Present border cells hold the unbanded closed forms.
  record: score / read_end / ref_end over the present cells with i < Rp, j < Fp; gscore / gref_end over the present candidates
  -1 <= j < Fp of row Rp - 1 -- none present: gscore = UNREACHED, gref_end = 0.  Rp = 0: five zeros.

X[:, i + 1, j + 1] is the definition's X(i, j): index 0 of either axis is the border (-1).
"""
import numpy as np

from extend_ref import _CLASS, trimmed_lengths

BLOCK_ROWS = 8                  # the library's B
UNREACHED = -(1 << 31)          # VALIGN_HIP_EXTEND_UNREACHED
_NEVER = -(1 << 40)             # an absent cell, and a gap state that does not exist
_LOST = _NEVER // 2             # anything below derives from an absent value


def present(R, F, band_width, B=BLOCK_ROWS):
    """-> bool [R + 1, F + 1]: the present cells, borders included (index 0 of either axis is -1)"""
    w = int(band_width) // 2
    P = np.zeros((R + 1, F + 1), bool)
    j = np.arange(-1, F)
    P[0] = j + 1 <= w
    for i in range(R):
        lo = B * (i // B) - w
        P[i + 1] = (lo <= j) & (j <= lo + B - 1 + 2 * w)
    return P


def unreached(Rp, Fp, band_width, B=BLOCK_ROWS):
    """the closed form: row Rp - 1 has no present candidate -1 <= j < Fp"""
    return Rp > 0 and B * ((Rp - 1) // B) - int(band_width) // 2 > Fp - 1


def matrices(reads, refs, scoring, band_width, affine=False, B=BLOCK_ROWS):
    """-> X int64 [n, R + 1, F + 1], P bool [R + 1, F + 1]: the cells of tests/extend_ref.py's matrix that the band keeps; absent
    cells hold _NEVER"""
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n, R = reads.shape
    F = refs.shape[1]
    P = present(R, F, band_width, B)
    rc, fc = _CLASS[reads], _CLASS[refs]
    both = (rc[:, :, None] > 0) & (fc[:, None, :] > 0)
    S = np.where(both, np.where(rc[:, :, None] == fc[:, None, :], int(scoring.match), int(scoring.mismatch)), 0).astype(np.int64)
    if affine:
        o_r, e_r, o_f, e_f = int(scoring.open_read), int(scoring.ext_read), int(scoring.open_ref), int(scoring.ext_ref)
    else:
        o_r = e_r = int(scoring.gap_read)
        o_f = e_f = int(scoring.gap_ref)
    X = np.full((n, R + 1, F + 1), _NEVER, np.int64)
    E = np.full((n, R + 1, F + 1), _NEVER, np.int64)
    G = np.full((n, R + 1, F + 1), _NEVER, np.int64)
    X[:, 0, 0] = 0
    X[:, 0, 1:] = np.where(P[0, 1:], o_r + e_r * np.arange(F), _NEVER)
    X[:, 1:, 0] = np.where(P[1:, 0], o_f + e_f * np.arange(R), _NEVER)[None, :]
    for d in range(2, R + F + 1):
        i = np.arange(max(1, d - F), min(R, d - 1) + 1)
        j = d - i
        keep = P[i, j]
        i, j = i[keep], j[keep]
        if i.size == 0:
            continue
        diag = X[:, i - 1, j - 1] + S[:, i - 1, j - 1]
        e = np.maximum(E[:, i, j - 1] + e_r, X[:, i, j - 1] + o_r)
        g = np.maximum(G[:, i - 1, j] + e_f, X[:, i - 1, j] + o_f)
        x = np.maximum(diag, np.maximum(e, g))
        assert (x > _LOST).all(), "a present cell without a present candidate"
        E[:, i, j] = np.where(e > _LOST, e, _NEVER)         # (an absent source stays absent: nothing drifts)
        G[:, i, j] = np.where(g > _LOST, g, _NEVER)
        X[:, i, j] = x
    return X, P


def record(X, P, Rp, Fp):
    """The record of ONE pair from its cells, row by row in plain Python: X int64 [R + 1, F + 1], P the present cells
    -> [score, read_end, ref_end, gscore, gref_end]"""
    if Rp == 0:
        return [0, 0, 0, 0, 0]
    best, bi, bj = 0, 0, 0
    for i in range(Rp):
        for j in range(Fp):
            if P[i + 1, j + 1] and X[i + 1, j + 1] > best:
                best, bi, bj = int(X[i + 1, j + 1]), i + 1, j + 1
    g, gj = None, 0
    for j in range(-1, Fp):
        if P[Rp, j + 1] and (g is None or X[Rp, j + 1] > g):
            g, gj = int(X[Rp, j + 1]), j + 1
    if g is None:
        g, gj = UNREACHED, 0
    return [best, bi, bj, g, gj]


def extend(reads, refs, scoring, band_width, affine=False, B=BLOCK_ROWS, chunk=256):
    """-> int64 [n, 5]: score, read_end, ref_end, gscore, gref_end under the band"""
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n, R = reads.shape
    F = refs.shape[1]
    out = np.zeros((n, 5), np.int64)
    Rp_all, Fp_all = trimmed_lengths(reads), trimmed_lengths(refs)
    rows, cols = np.arange(R)[None, :, None], np.arange(F)[None, None, :]
    for b in range(0, n, chunk):
        X, P = matrices(reads[b:b + chunk], refs[b:b + chunk], scoring, band_width, affine, B)
        m = len(X)
        Rp, Fp = Rp_all[b:b + chunk], Fp_all[b:b + chunk]
        inside = (rows < Rp[:, None, None]) & (cols < Fp[:, None, None]) & P[None, 1:, 1:]
        flat = np.where(inside, X[:, 1:, 1:], _NEVER).reshape(m, -1)
        if flat.shape[1]:
            at = flat.argmax(axis=1)                    # the first occurrence in row-major order
            best = flat[np.arange(m), at]
            hit = best > 0
            out[b:b + chunk, 0] = np.where(hit, best, 0)
            out[b:b + chunk, 1] = np.where(hit, at // F + 1, 0)
            out[b:b + chunk, 2] = np.where(hit, at % F + 1, 0)
        row = np.maximum(Rp, 1)
        last = X[np.arange(m), row, :]                  # row Rp - 1, border column first
        cand = (np.arange(F + 1)[None, :] <= Fp[:, None]) & P[row, :]
        last = np.where(cand, last, _NEVER)
        gat = last.argmax(axis=1)                       # the smallest candidate column
        has, reached = Rp > 0, cand.any(axis=1)
        out[b:b + chunk, 3] = np.where(has, np.where(reached, last[np.arange(m), gat], UNREACHED), 0)
        out[b:b + chunk, 4] = np.where(has & reached, gat, 0)
    return out
