"""Z-dropped extension scores (include/valign_hip.h: valign_hip_set_extend_zdrop) restated in numpy and plain Python, independent
of the library.  No cell changes: the matrix is tests/extend_band_ref.py's (int64 cells, absent cells a value no maximum takes; a
band of 2 * max(R, F) + 2 keeps every cell and gives the unbanded matrix).  Only which rows count changes:

  row maxima    m_i = the maximum of X(i, j) over the present candidates -1 <= j < Fp of row i < Rp (the border column counts),
                c_i the smallest such column.  A row without a present candidate is skipped: it neither updates nor drops.
  running best  (M, Mi, Mj) = (0, -1, -1), the anchor.  Rows in order: m_i > M moves it to (m_i, i, c_i); otherwise, with
                di = i - Mi, dj = c_i - Mj and pen = (di - dj) * |ext_ref| if di > dj else (dj - di) * |ext_read| (linear gaps:
                gap_ref, gap_read), the row DROPS iff M - m_i - pen > Z (Python integers: nothing wraps).
  drop row      T = the first dropping row, Rp if none drops.
  record        score = M, read_end = Mi + 1, ref_end = Mj + 1 as they stand at T (three zeros for M = 0); T == Rp: gscore / gref_end
                of the matrix, the band's unreached read end included; T < Rp: gscore = UNREACHED, gref_end = 0.  Rp = 0: five zeros.

Alignments under the key (the banded route): the alignment of the pair CUT to its first T rows, ending in its best cell -- never in
its read end where T < Rp.  That is the same alignment because a cell depends on the cells above and left of it only, so the rows
before T hold the same values with or without the rows from T on; the record's cell is the row-major first maximum over the rows
before T, which is the cut pair's best cell; and the walk from it only moves up and left.
"""
import numpy as np

import extend_band_ref as ebr
from extend_ref import trimmed_lengths

UNREACHED = ebr.UNREACHED
STRIP_ROWS = 512                # a strip of the int32 extension sweep
NEVER_DROPS = 1 << 29           # Z from here on drops no row (include/valign_hip.h)


def prices(scoring, affine):
    """-> |ext_ref|, |ext_read| (linear gaps: |gap_ref|, |gap_read|)"""
    if affine:
        return abs(int(scoring.ext_ref)), abs(int(scoring.ext_read))
    return abs(int(scoring.gap_ref)), abs(int(scoring.gap_read))


def row_maxima(X, P, Rp, Fp):
    """ONE pair -> a list of (i, m_i, c_i) over the rows i < Rp that have a present candidate -1 <= j < Fp"""
    out = []
    for i in range(Rp):
        keep = np.nonzero(P[i + 1, :Fp + 1])[0]
        if keep.size == 0:
            continue
        vals = X[i + 1, keep]
        at = int(vals.argmax())                         # the first occurrence: the smallest column
        out.append((i, int(vals[at]), int(keep[at]) - 1))
    return out


def drop(rows, Rp, Z, price_ref, price_read):
    """The row loop of the definition -> (M, Mi, Mj) at T, and T"""
    M, Mi, Mj = 0, -1, -1
    for i, m, c in rows:
        if m > M:
            M, Mi, Mj = m, i, c
            continue
        di, dj = i - Mi, c - Mj
        pen = (di - dj) * price_ref if di > dj else (dj - di) * price_read
        if M - m - pen > Z:
            return (M, Mi, Mj), i
    return (M, Mi, Mj), Rp


def record(X, P, Rp, Fp, Z, price_ref, price_read):
    """ONE pair -> [score, read_end, ref_end, gscore, gref_end], T"""
    if Rp == 0:
        return [0, 0, 0, 0, 0], 0
    (M, Mi, Mj), T = drop(row_maxima(X, P, Rp, Fp), Rp, Z, price_ref, price_read)
    if T < Rp:
        return [M, Mi + 1, Mj + 1, UNREACHED, 0], T
    whole = ebr.record(X, P, Rp, Fp)
    return [M, Mi + 1, Mj + 1, whole[3], whole[4]], T


def extend(reads, refs, scoring, Z, band_width=0, affine=False, chunk=16):
    """-> records int64 [n, 5], T int64 [n].  band_width = 0: unbanded"""
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n, R = reads.shape
    F = refs.shape[1]
    band = band_width if band_width > 0 else 2 * max(R, F) + 2
    p_ref, p_read = prices(scoring, affine)
    Rp, Fp = trimmed_lengths(reads), trimmed_lengths(refs)
    out, T = np.zeros((n, 5), np.int64), np.zeros(n, np.int64)
    for b in range(0, n, chunk):
        X, P = ebr.matrices(reads[b:b + chunk], refs[b:b + chunk], scoring, band, affine)
        for k in range(len(X)):
            out[b + k], T[b + k] = record(X[k], P, int(Rp[b + k]), int(Fp[b + k]), Z, p_ref, p_read)
    return out, T


def skipped_waves(T, Rp, Fp, R, band_width):
    """The waves of a call that skip a strip: a wave is two consecutive pairs (the last one alone where n is odd), a strip 512 rows.
    Strip s > 0 is skipped where both pairs dropped above it (T < Rp and T < 512 s) -- counted only where the strip would have run:
    some row of the wave below 512 s and, under a band, a window with a column below the wave's larger Fp."""
    T, Rp, Fp = (np.asarray(a, np.int64) for a in (T, Rp, Fp))
    w = int(band_width) // 2
    count = 0
    for s in range(1, (R + STRIP_ROWS - 1) // STRIP_ROWS):
        row0 = s * STRIP_ROWS
        for a in range(0, len(T), 2):
            pair = [a, a + 1 if a + 1 < len(T) else a]
            if Rp[pair].max() <= row0:
                continue
            if band_width > 0 and max(row0 - w, 0) >= min(row0 + STRIP_ROWS + w, int(Fp[pair].max())):
                continue
            if all(T[p] < Rp[p] and T[p] < row0 for p in pair):
                count += 1
    return count


def cut_reads(reads, T):
    """the pairs cut to their first T rows (the rest N): what an alignment under the key is the alignment of"""
    cut = np.array(reads, np.uint8, copy=True)
    for k, t in enumerate(T):
        cut[k, int(t):] = ord("N")
    return cut
