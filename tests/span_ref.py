"""Spanned Smith-Waterman scores (include/valign_hip.h: valign_hip_span) restated in numpy, independent of the library and of
the oracle's C, and UNCLIPPED: the reverse sweep runs over the whole reversed prefixes.

  score, read_end, ref_end: placed_ref.placed.  Then both prefixes read[0, read_end) and ref[0, ref_end) are reversed, the same
  Smith-Waterman matrix (placed_ref.matrices: same scoring, same gap model, read steps and reference steps keeping their roles)
  is filled over them, and the first cell in row-major order that holds `score` -- (i', j'), 0-based -- gives
  read_begin = read_end - 1 - i', ref_begin = ref_end - 1 - j'.  A pair whose maximum is 0 is five zeros.

The reversed prefixes of a batch have different lengths: they are laid out left-aligned in arrays of the full shape, and the
cells outside a pair's own (read_end x ref_end) rectangle are masked out before anything is read -- a cell depends on the cells
above and left of it only, so what lies in the padding never reaches a cell that is read.

global_scores is the check of the guarantee: a plain global (end-to-end) alignment score of the span under the same scoring,
written on its own recurrences (no floor at 0, gap borders)."""
import numpy as np

import placed_ref

NEG = -(1 << 40)


def _reversed_prefixes(seqs, ends):
    """[n, L] bytes, ends [n] -> [n, L]: row p holds seqs[p, :ends[p]] reversed, then NUL"""
    n, L = seqs.shape
    k = np.arange(L)[None, :]
    src = ends[:, None] - 1 - k
    ok = src >= 0
    out = np.take_along_axis(seqs, np.where(ok, src, 0), axis=1)
    return np.where(ok, out, 0).astype(np.uint8)


def reverse_matrices(reads, refs, placed, scoring, affine=False, clip=None):
    """-> (H of the reversed prefixes [n, R, Fc] with every cell outside the pair's own rectangle set to -1, Fc): Fc = F, or
    `clip` columns of the reversed reference where given"""
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n, R = reads.shape
    F = refs.shape[1]
    rr = _reversed_prefixes(reads, placed[:, 1])
    rf = _reversed_prefixes(refs, placed[:, 2])
    Fc = F if clip is None else min(F, int(clip))
    rf = rf[:, :Fc]
    H = placed_ref.matrices(rr, rf, scoring, affine)[:, 1:, 1:]
    inside = (np.arange(R)[None, :, None] < placed[:, 1][:, None, None]) & (np.arange(Fc)[None, None, :] < placed[:, 2][:, None, None])
    return np.where(inside, H, -1), Fc


def spans(reads, refs, scoring, affine=False, clip=None, chunk=256, with_reverse_max=False):
    """-> int64 [n, 5]: score, read_begin, read_end, ref_begin, ref_end (0-based, half-open; zeros where the maximum is 0);
    with_reverse_max: also the maximum of every pair's reversed matrix (0 for an empty pair)"""
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n = len(reads)
    out = np.zeros((n, 5), np.int64)
    rev_max = np.zeros(n, np.int64)
    for b in range(0, n, chunk):
        pl = placed_ref.placed(reads[b:b + chunk], refs[b:b + chunk], scoring, affine)
        H, Fc = reverse_matrices(reads[b:b + chunk], refs[b:b + chunk], pl, scoring, affine, clip)
        flat = H.reshape(len(H), -1)
        if flat.shape[1] == 0:
            continue
        hit = pl[:, 0] > 0
        rev_max[b:b + chunk] = np.where(hit, flat.max(axis=1), 0)
        at = (flat == pl[:, :1]).argmax(axis=1)                     # the first cell in row-major order that holds `score`
        found = flat[np.arange(len(H)), at] == pl[:, 0]
        assert (found | ~hit).all(), "a reversed matrix does not hold the forward score"
        i, j = at // Fc, at % Fc
        out[b:b + chunk, 0] = np.where(hit, pl[:, 0], 0)
        out[b:b + chunk, 1] = np.where(hit, pl[:, 1] - 1 - i, 0)
        out[b:b + chunk, 2] = np.where(hit, pl[:, 1], 0)
        out[b:b + chunk, 3] = np.where(hit, pl[:, 2] - 1 - j, 0)
        out[b:b + chunk, 4] = np.where(hit, pl[:, 2], 0)
    return (out, rev_max) if with_reverse_max else out


def _suffixes(seqs, begins):
    n, L = seqs.shape
    src = begins[:, None] + np.arange(L)[None, :]
    ok = src < L
    return np.where(ok, np.take_along_axis(seqs, np.where(ok, src, 0), axis=1), 0).astype(np.uint8)


def global_scores(reads, refs, recs, scoring, affine=False):
    """The global alignment score of read[read_begin, read_end) against ref[ref_begin, ref_end) of every record (0 for an empty
    one): every base of both spans is aligned or gapped, nothing is free.  -> int64 [n]"""
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n, R = reads.shape
    F = refs.shape[1]
    sr = _suffixes(reads, recs[:, 1])
    sf = _suffixes(refs, recs[:, 3])
    cls = placed_ref._CLASS
    rc, fc = cls[sr], cls[sf]
    both = (rc[:, :, None] > 0) & (fc[:, None, :] > 0)
    S = np.where(both, np.where(rc[:, :, None] == fc[:, None, :], int(scoring.match), int(scoring.mismatch)), 0).astype(np.int64)
    H = np.full((n, R + 1, F + 1), NEG, np.int64)
    H[:, 0, 0] = 0
    jj, ii = np.arange(1, F + 1), np.arange(1, R + 1)
    if affine:
        o_r, e_r, o_f, e_f = int(scoring.open_read), int(scoring.ext_read), int(scoring.open_ref), int(scoring.ext_ref)
        E = np.full((n, R + 1, F + 1), NEG, np.int64)       # ends in a reference base against a gap in the read
        G = np.full((n, R + 1, F + 1), NEG, np.int64)       # ends in a read base against a gap in the reference
        H[:, 0, 1:] = E[:, 0, 1:] = o_r + (jj - 1) * e_r
        H[:, 1:, 0] = G[:, 1:, 0] = (o_f + (ii - 1) * e_f)[None, :]
    else:
        g_r, g_f = int(scoring.gap_read), int(scoring.gap_ref)
        H[:, 0, 1:] = jj * g_r
        H[:, 1:, 0] = (ii * g_f)[None, :]
    for d in range(2, R + F + 1):
        i = np.arange(max(1, d - F), min(R, d - 1) + 1)
        j = d - i
        diag = H[:, i - 1, j - 1] + S[:, i - 1, j - 1]
        if affine:
            e = np.maximum(E[:, i, j - 1] + e_r, H[:, i, j - 1] + o_r)
            g = np.maximum(G[:, i - 1, j] + e_f, H[:, i - 1, j] + o_f)
            E[:, i, j] = e
            G[:, i, j] = g
            H[:, i, j] = np.maximum(diag, np.maximum(e, g))
        else:
            H[:, i, j] = np.maximum(diag, np.maximum(H[:, i, j - 1] + g_r, H[:, i - 1, j] + g_f))
    return H[np.arange(n), recs[:, 2] - recs[:, 1], recs[:, 4] - recs[:, 3]]
