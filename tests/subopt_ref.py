"""Suboptimal Smith-Waterman scores (include/valign_hip.h: valign_hip_subopt) restated in numpy on placed_ref.matrices,
independent of the library: the placed record, then the largest column maximum -- over the rows below the trimmed read length
and the columns below the trimmed reference length -- at more than `mask` columns from the end cell, and the smallest column
that holds it."""
import numpy as np

import placed_ref


def trimmed_lengths(seqs):
    """-> int64 [n]: 1 + the position of the last ACGT byte (either case) of each row, 0 where there is none"""
    good = placed_ref._CLASS[np.asarray(seqs, np.uint8)] > 0
    n, L = good.shape
    return np.where(good.any(axis=1), L - np.argmax(good[:, ::-1], axis=1), 0).astype(np.int64)


def column_maxima(reads, refs, scoring, affine=False, trim_rows=True):
    """-> int64 [n, F]: colmax[j] over the rows below the trimmed read length (trim_rows False: over all rows)"""
    H = placed_ref.matrices(reads, refs, scoring, affine)[:, 1:, 1:]
    if trim_rows and H.shape[1]:
        Rp = trimmed_lengths(reads)
        H = np.where(np.arange(H.shape[1])[None, :, None] < Rp[:, None, None], H, 0)
    return H.max(axis=1) if H.shape[1] else np.zeros((H.shape[0], H.shape[2]), np.int64)


def prepare(reads, refs, scoring, affine=False, chunk=256, trim=True):
    """-> (placed int64 [n, 3], colmax int64 [n, F], Fp int64 [n]): everything of the definition that does not read the mask"""
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n, F = len(reads), refs.shape[1]
    cm = np.zeros((n, F), np.int64)
    for b in range(0, n, chunk):
        cm[b:b + chunk] = column_maxima(reads[b:b + chunk], refs[b:b + chunk], scoring, affine, trim_rows=trim)
    Fp = trimmed_lengths(refs) if trim else np.full(n, F, np.int64)
    return placed_ref.placed(reads, refs, scoring, affine, chunk), cm, Fp


def apply_mask(prepared, mask):
    """-> int64 [n, 5]: score, read_end, ref_end, score2, ref_end2 for this mask"""
    rec, cm, Fp = prepared
    n, F = cm.shape
    out = np.zeros((n, 5), np.int64)
    out[:, :3] = rec
    if F == 0:
        return out
    cols = np.arange(F)[None, :]
    cand = (np.abs(cols - (rec[:, 2:3] - 1)) > int(mask)) & (cols < Fp[:, None]) & (rec[:, 0:1] > 0)
    cm = np.where(cand, cm, 0)
    at = cm.argmax(axis=1)                          # the first occurrence: the smallest column
    best = cm[np.arange(n), at]
    out[:, 3] = best
    out[:, 4] = np.where(best > 0, at + 1, 0)
    return out


def subopt(reads, refs, scoring, mask, affine=False, chunk=256, trim=True):
    """-> int64 [n, 5]: score, read_end, ref_end, score2, ref_end2.  trim False: every row and column is a candidate (what
    the definition does NOT say; the tests show why)"""
    return apply_mask(prepare(reads, refs, scoring, affine, chunk, trim), mask)
