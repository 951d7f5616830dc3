"""Extension scores (include/valign_hip.h: valign_hip_extend) restated in numpy, independent of the library: the whole matrix on
int64 cells for both gap models, anchored at the origin -- gap-priced borders, no floor at zero -- filled anti-diagonal by
anti-diagonal for the whole batch at once, then the record.

  scoring: an object with match, mismatch, gap_read, gap_ref, open_read, ext_read, open_ref, ext_ref (hipkernel.Scoring,
  oracle.cpu_ref.Scoring).  Two bases score match / mismatch when both are one of ACGT (either case), anything else scores 0.
  A step along the row (a reference base against a gap in the read) costs gap_read (affine: open_read, then ext_read), a step
  down the column gap_ref (open_ref, then ext_ref).

X[:, i + 1, j + 1] is the definition's X(i, j): index 0 of either axis is the border (-1).
"""
import numpy as np

_CLASS = np.zeros(256, np.int64)
for _k, _ch in enumerate("ACGT"):
    _CLASS[ord(_ch)] = _CLASS[ord(_ch.lower())] = _k + 1

_NEVER = -(1 << 40)          # a value no maximum takes: a gap state that does not exist on a border


def trimmed_lengths(seqs):
    """-> int64 [n]: 1 + the position of the last ACGT byte (either case) of each row, 0 where there is none"""
    good = _CLASS[np.asarray(seqs, np.uint8)] > 0
    n, L = good.shape
    if L == 0:
        return np.zeros(n, np.int64)
    return np.where(good.any(axis=1), L - np.argmax(good[:, ::-1], axis=1), 0).astype(np.int64)


def matrices(reads, refs, scoring, affine=False):
    """-> X int64 [n, R + 1, F + 1]: X(-1, -1) = 0, the border column a gap of i + 1 read bases, the border row a gap of j + 1
    reference bases, inside the linear or Gotoh recurrence without a floor"""
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n, R = reads.shape
    F = refs.shape[1]
    rc, fc = _CLASS[reads], _CLASS[refs]
    both = (rc[:, :, None] > 0) & (fc[:, None, :] > 0)
    S = np.where(both, np.where(rc[:, :, None] == fc[:, None, :], int(scoring.match), int(scoring.mismatch)), 0).astype(np.int64)
    if affine:
        o_r, e_r, o_f, e_f = int(scoring.open_read), int(scoring.ext_read), int(scoring.open_ref), int(scoring.ext_ref)
    else:       # a linear gap is an affine one whose opening costs what an extension does
        o_r = e_r = int(scoring.gap_read)
        o_f = e_f = int(scoring.gap_ref)
    X = np.zeros((n, R + 1, F + 1), np.int64)
    E = np.full((n, R + 1, F + 1), _NEVER, np.int64)        # best value ending in a step along the row
    G = np.full((n, R + 1, F + 1), _NEVER, np.int64)        # ... down the column
    X[:, 0, 1:] = o_r + e_r * np.arange(F)           # (a gap run that turns the corner opens again: E and G stay unset on the borders)
    X[:, 1:, 0] = (o_f + e_f * np.arange(R))[None, :]
    for d in range(2, R + F + 1):
        i = np.arange(max(1, d - F), min(R, d - 1) + 1)
        j = d - i
        diag = X[:, i - 1, j - 1] + S[:, i - 1, j - 1]
        e = np.maximum(E[:, i, j - 1] + e_r, X[:, i, j - 1] + o_r)
        g = np.maximum(G[:, i - 1, j] + e_f, X[:, i - 1, j] + o_f)
        E[:, i, j] = e
        G[:, i, j] = g
        X[:, i, j] = np.maximum(diag, np.maximum(e, g))
    return X


def record(X, Rp, Fp):
    """The record of ONE pair from its cells: X int64 [R + 1, F + 1] (or anything indexed the same way), trimmed lengths Rp, Fp
    -> [score, read_end, ref_end, gscore, gref_end]"""
    if Rp == 0:
        return [0, 0, 0, 0, 0]
    best, bi, bj = 0, 0, 0
    for i in range(Rp):
        for j in range(Fp):
            if X[i + 1, j + 1] > best:          # row-major, strictly greater: the first cell that holds the maximum
                best, bi, bj = int(X[i + 1, j + 1]), i + 1, j + 1
    g, gj = int(X[Rp, 0]), 0                    # the border column is candidate j = -1
    for j in range(Fp):
        if X[Rp, j + 1] > g:
            g, gj = int(X[Rp, j + 1]), j + 1
    return [best, bi, bj, g, gj]


def extend(reads, refs, scoring, affine=False, chunk=256):
    """-> int64 [n, 5]: score, read_end, ref_end, gscore, gref_end"""
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n, R = reads.shape
    F = refs.shape[1]
    out = np.zeros((n, 5), np.int64)
    Rp_all, Fp_all = trimmed_lengths(reads), trimmed_lengths(refs)
    rows, cols = np.arange(R)[None, :, None], np.arange(F)[None, None, :]
    for b in range(0, n, chunk):
        X = matrices(reads[b:b + chunk], refs[b:b + chunk], scoring, affine)
        m = len(X)
        Rp, Fp = Rp_all[b:b + chunk], Fp_all[b:b + chunk]
        inside = (rows < Rp[:, None, None]) & (cols < Fp[:, None, None])
        flat = np.where(inside, X[:, 1:, 1:], _NEVER).reshape(m, -1)
        if flat.shape[1]:
            at = flat.argmax(axis=1)                    # the first occurrence in row-major order
            best = flat[np.arange(m), at]
            hit = best > 0
            out[b:b + chunk, 0] = np.where(hit, best, 0)
            out[b:b + chunk, 1] = np.where(hit, at // F + 1, 0)
            out[b:b + chunk, 2] = np.where(hit, at % F + 1, 0)
        last = X[np.arange(m), np.maximum(Rp, 1), :]                         # row Rp - 1, border column first
        last = np.where(np.arange(F + 1)[None, :] <= Fp[:, None], last, _NEVER)
        gat = last.argmax(axis=1)                       # the smallest candidate column
        has = Rp > 0
        out[b:b + chunk, 3] = np.where(has, last[np.arange(m), gat], 0)
        out[b:b + chunk, 4] = np.where(has, gat, 0)
    return out
