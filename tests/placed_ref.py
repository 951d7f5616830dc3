"""Placed Smith-Waterman scores (include/valign_hip.h: valign_hip_placed) restated in numpy, independent of the library and of
the oracle's C: the full matrix on int64 cells, linear gaps or affine gaps (Gotoh, the project's model: a run of k gap bases
costs open + (k - 1) * extend, per direction), filled anti-diagonal by anti-diagonal for the whole batch at once, then the
first cell in row-major order that holds the maximum -- the reference's "first cell strictly greater than every earlier one"
(src/Kernels/default/DefaultKernel.cpp:252-256).

  scoring: an object with match, mismatch, gap_read, gap_ref, open_read, ext_read, open_ref, ext_ref (oracle.cpu_ref.Scoring,
  hipkernel.Scoring).  Two bases score match / mismatch when both are one of ACGT (either case), anything else scores 0.
  A step along the row (a reference base against a gap in the read) costs gap_read (affine: open_read / ext_read), a step
  down the column gap_ref (open_ref / ext_ref).
"""
import numpy as np

_CLASS = np.zeros(256, np.int64)
for _k, _ch in enumerate("ACGT"):
    _CLASS[ord(_ch)] = _CLASS[ord(_ch.lower())] = _k + 1


def matrices(reads, refs, scoring, affine=False):
    """-> H int64 [n, R + 1, F + 1] (row 0 and column 0 are the zero border)"""
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n, R = reads.shape
    F = refs.shape[1]
    rc, fc = _CLASS[reads], _CLASS[refs]
    both = (rc[:, :, None] > 0) & (fc[:, None, :] > 0)
    S = np.where(both, np.where(rc[:, :, None] == fc[:, None, :], int(scoring.match), int(scoring.mismatch)), 0).astype(np.int64)
    H = np.zeros((n, R + 1, F + 1), np.int64)
    if affine:
        E = np.zeros((n, R + 1, F + 1), np.int64)       # best value ending in a step along the row
        G = np.zeros((n, R + 1, F + 1), np.int64)       # ... down the column
        o_r, e_r, o_f, e_f = int(scoring.open_read), int(scoring.ext_read), int(scoring.open_ref), int(scoring.ext_ref)
    else:
        g_r, g_f = int(scoring.gap_read), int(scoring.gap_ref)
    for d in range(2, R + F + 1):
        i = np.arange(max(1, d - F), min(R, d - 1) + 1)
        j = d - i
        diag = H[:, i - 1, j - 1] + S[:, i - 1, j - 1]
        if affine:
            e = np.maximum(np.maximum(E[:, i, j - 1] + e_r, H[:, i, j - 1] + o_r), 0)
            g = np.maximum(np.maximum(G[:, i - 1, j] + e_f, H[:, i - 1, j] + o_f), 0)
            E[:, i, j] = e
            G[:, i, j] = g
            H[:, i, j] = np.maximum(np.maximum(diag, e), np.maximum(g, 0))
        else:
            H[:, i, j] = np.maximum(np.maximum(diag, H[:, i, j - 1] + g_r), np.maximum(H[:, i - 1, j] + g_f, 0))
    return H


def placed(reads, refs, scoring, affine=False, chunk=256):
    """-> int64 [n, 3]: score, read_end, ref_end (0-based, half-open; all zeros where the maximum is 0)"""
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n, F = len(reads), refs.shape[1]
    out = np.zeros((n, 3), np.int64)
    for b in range(0, n, chunk):
        H = matrices(reads[b:b + chunk], refs[b:b + chunk], scoring, affine)[:, 1:, 1:]
        flat = H.reshape(len(H), -1)
        if flat.shape[1] == 0:
            continue
        at = flat.argmax(axis=1)                       # the first occurrence in row-major order
        best = flat[np.arange(len(H)), at]
        hit = best > 0
        out[b:b + chunk, 0] = np.where(hit, best, 0)
        out[b:b + chunk, 1] = np.where(hit, at // F + 1, 0)
        out[b:b + chunk, 2] = np.where(hit, at % F + 1, 0)
    return out
