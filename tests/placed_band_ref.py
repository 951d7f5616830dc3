"""Banded placed Smith-Waterman scores (include/valign_hip.h: valign_hip_set_band_placed) restated in numpy, independent of the
library and of the oracle's C.

Definition: row i of the read has the inclusive column window band_align_ref.row_window(i, R, F, band_width, 16, 1) -- the
chain's block band --; every cell outside its row's window holds 0 (affine: H, E and F alike).  Inside, the recurrence of
tests/placed_ref.py on int64 cells: linear gaps, or Gotoh in the project's model (a run of k gap bases costs open + (k - 1) *
extend, per direction; E and F floored at 0 like H).  The record is the first cell in row-major order whose value is strictly
greater than every earlier one (src/Kernels/default/DefaultKernel.cpp:252-256), over in-band cells: score, read_end, ref_end
(0-based, half-open), {0, 0, 0} where the maximum is 0.

Rows are filled one by one for the whole batch; the dependency along a row is a running maximum: with c <= 0 the cost of one
more step, X[j] = max(A[j], X[j - 1] + c) is max_k<=j (A[k] - k c) + j c.
"""
import numpy as np

from band_align_ref import row_window

_CLASS = np.zeros(256, np.int64)
for _k, _ch in enumerate("ACGT"):
    _CLASS[ord(_ch)] = _CLASS[ord(_ch.lower())] = _k + 1

BLOCK_ROWS, COL_ALIGN = 16, 1


def placed_banded(reads, refs, band_width, scoring, affine=False):
    """-> int64 [n, 3]: score, read_end, ref_end of the banded placed score of every pair"""
    reads = np.ascontiguousarray(reads, np.uint8)
    refs = np.ascontiguousarray(refs, np.uint8)
    n, R = reads.shape
    F = refs.shape[1]
    rc, fc = _CLASS[reads], _CLASS[refs]
    match, mismatch = int(scoring.match), int(scoring.mismatch)
    if affine:
        o_r, e_r, o_f, e_f = int(scoring.open_read), int(scoring.ext_read), int(scoring.open_ref), int(scoring.ext_ref)
    else:
        g_r, g_f = int(scoring.gap_read), int(scoring.gap_ref)
    # the row above at index j + 1 (index 0: the border column), 0 outside its window
    h_prev = np.zeros((n, F + 1), np.int64)
    g_prev = np.zeros((n, F + 1), np.int64)            # affine: best value ending in a step down the column
    best = np.zeros(n, np.int64)
    best_i = np.zeros(n, np.int64)
    best_j = np.zeros(n, np.int64)
    for i in range(R):
        lo, hi = row_window(i, R, F, band_width, BLOCK_ROWS, COL_ALIGN)
        if lo > hi:
            h_prev = np.zeros((n, F + 1), np.int64)
            g_prev = np.zeros((n, F + 1), np.int64)
            continue
        js = np.arange(lo, hi + 1)
        a, b = rc[:, i:i + 1], fc[:, lo:hi + 1]
        s = np.where((a > 0) & (b > 0), np.where(a == b, match, mismatch), 0)
        diag = h_prev[:, lo:hi + 1] + s
        up = h_prev[:, lo + 1:hi + 2]
        if affine:
            g = np.maximum(np.maximum(g_prev[:, lo + 1:hi + 2] + e_f, up + o_f), 0)
            base = np.maximum(np.maximum(diag, g), 0)
            # E[j] = max(0, H[j - 1] + o_r, E[j - 1] + e_r), H = max(base, E): E[j] = max(0, base[j - 1] + o_r, E[j - 1] + c),
            # c = max(e_r, o_r); E[lo] = 0 (its left neighbour is outside)
            c = max(e_r, o_r)
            x = np.zeros_like(base)
            x[:, 1:] = np.maximum(base[:, :-1] + o_r, 0)
            e = np.maximum.accumulate(x - js * c, axis=1) + js * c
            h = np.maximum(base, e)
            g_prev = np.zeros((n, F + 1), np.int64)
            g_prev[:, lo + 1:hi + 2] = g
        else:
            base = np.maximum(np.maximum(diag, up + g_f), 0)
            h = np.maximum.accumulate(base - js * g_r, axis=1) + js * g_r
        row_max = h.max(axis=1)
        better = row_max > best                          # strictly: an earlier row keeps a tie
        arg = h.argmax(axis=1)                           # the first column of the row that holds it
        best = np.where(better, row_max, best)
        best_i = np.where(better, i, best_i)
        best_j = np.where(better, lo + arg, best_j)
        h_prev = np.zeros((n, F + 1), np.int64)
        h_prev[:, lo + 1:hi + 2] = h
    hit = best > 0
    return np.stack([np.where(hit, best, 0), np.where(hit, best_i + 1, 0), np.where(hit, best_j + 1, 0)], axis=1)
