"""Banded Smith-Waterman alignments, restated in numpy (a helper of the tests, vectorised over pairs).

Definition (include/valign_hip.h, band_alignments): the reference's Default SW fill and traceback (DefaultKernel.cpp:204-280,
391-456) on int32 cells, on the block band of band_width (oracle/cpu_ref.c band_columns with block_rows / col_align):
  * every cell outside its row's window holds 0 (affine: H = E = F = 0) with pointer START;
  * linear gaps: pointer DIAG > UP > LEFT, START where the cell is 0; affine gaps: the Gotoh recurrence of
    vref_score_banded_sw_affine (E and F floored at 0 like H), H from DIAG > F > E, a gap opened rather than extended on ties;
  * the end cell is the row-major first strict maximum over in-band cells;
  * the walk stops at START, or at a step that leaves the band.
Rows and coordinates come back in cpu_ref.align's layout: rows uint8 [n, 2, R + F] right-justified behind zeros (NUL at
R + F - 1), idx int16 [n, 4] = readStart, readEnd, refStart, refEnd.
"""
import numpy as np

_CLASS = np.zeros(256, np.int64)
for _c, _v in zip(b"ATCGN", (1, 2, 3, 4, 5)):
    _CLASS[_c] = _v
    _CLASS[ord(chr(_c).lower())] = _v
_START, _DIAG, _UP, _LEFT = 3, 0, 1, 2          # linear codes; affine H codes: 0 DIAG, 1 from F, 2 from E, 3 START


def row_window(i, R, F, band_width, block_rows, col_align):
    """[lo, hi] (inclusive) of read row i: oracle/cpu_ref.c band_columns."""
    w = band_width // 2
    blocks = (R + block_rows - 1) // block_rows
    pad = blocks * block_rows - R
    b = (i + pad) // block_rows
    r_lo = max(b * block_rows - pad, 0)
    r_hi = min((b + 1) * block_rows - pad - 1, R - 1)
    lo = max(r_lo * F // R - w, 0)
    lo -= lo % col_align
    hi = min(r_hi * F // R + w, F - 1)
    return lo, hi


def _scores(sc, reads, refs):
    tab = np.zeros((6, 6), np.int64)
    tab[1:5, 1:5] = sc.mismatch
    for a in range(1, 5):
        tab[a, a] = sc.match
    return tab, _CLASS[reads], _CLASS[refs]


def align_banded_sw(reads, refs, band_width, scoring, block_rows=1, col_align=1, affine=False, paths=False):
    """-> rows uint8 [n, 2, R + F], idx int16 [n, 4] of the banded SW alignments (module docstring); paths=True adds, per pair,
    the list of the (read, ref) cells the walk emitted."""
    reads = np.ascontiguousarray(reads, np.uint8)
    refs = np.ascontiguousarray(refs, np.uint8)
    n, R = reads.shape
    F = refs.shape[1]
    tab, rc, fc = _scores(scoring, reads, refs)
    gr, gf = scoring.gap_read, scoring.gap_ref
    oR, eR, oF, eF = scoring.open_read, scoring.ext_read, scoring.open_ref, scoring.ext_ref
    h_prev = np.zeros((n, F + 1), np.int64)          # H of the row above at column j - 1 (index j), 0 outside its window
    f_prev = np.zeros((n, F + 1), np.int64)
    best = np.zeros(n, np.int64)
    best_i = np.zeros(n, np.int64)
    best_j = np.zeros(n, np.int64)
    windows, codes, e_ext, f_ext = [], [], [], []
    ar = np.arange(n)
    for i in range(R):
        lo, hi = row_window(i, R, F, band_width, block_rows, col_align)
        js = np.arange(lo, hi + 1)
        d = h_prev[:, lo:hi + 1] + tab[rc[:, i:i + 1], fc[:, lo:hi + 1]]
        up = h_prev[:, lo + 1:hi + 2]
        if not affine:
            u = np.maximum(up + gf, 0)
            a = np.maximum(np.maximum(d, u), 0)
            # H[j] = max(A[j], H[j - 1] + gap_read), H[lo - 1] = 0 (outside): a running maximum
            h = np.maximum.accumulate(a - js * gr, axis=1) + js * gr
            code = np.where(h == d, _DIAG, np.where(h == u, _UP, _LEFT))
        else:
            f_open = np.maximum(up + oF, 0)
            f_extd = np.maximum(f_prev[:, lo + 1:hi + 2] + eF, 0)
            f = np.maximum(f_open, f_extd)
            b = np.maximum(np.maximum(d, f), 0)
            # E[j] = max(0, B[j - 1] + open_read, E[j - 1] + max(ext_read, open_read)), E[lo] = 0
            c = max(eR, oR)
            x = np.zeros_like(b)
            x[:, 1:] = np.maximum(b[:, :-1] + oR, 0)
            e = np.maximum.accumulate(x - js * c, axis=1) + js * c
            h = np.maximum(b, e)
            h_left = np.zeros_like(h)
            e_left = np.zeros_like(h)
            h_left[:, 1:] = h[:, :-1]
            e_left[:, 1:] = e[:, :-1]
            code = np.where(h == d, 0, np.where(h == f, 1, 2))
            e_ext.append(np.maximum(e_left + eR, 0) > np.maximum(h_left + oR, 0))
            f_ext.append(f_extd > f_open)
            f_prev = np.zeros((n, F + 1), np.int64)
            f_prev[:, lo + 1:hi + 2] = f
        code = np.where(h == 0, _START, code)
        windows.append((lo, hi))
        codes.append(code.astype(np.uint8))
        rmax = h.max(axis=1)
        better = rmax > best
        arg = h.argmax(axis=1)
        best = np.where(better, rmax, best)
        best_i = np.where(better, i, best_i)
        best_j = np.where(better, lo + arg, best_j)
        h_prev = np.zeros((n, F + 1), np.int64)
        h_prev[:, lo + 1:hi + 2] = h
    AL = R + F
    rows = np.zeros((n, 2, AL), np.uint8)
    idx = np.zeros((n, 4), np.int16)
    walked = [[] for _ in range(n)]
    for p in ar:
        i, j = int(best_i[p]), int(best_j[p])
        if best[p] <= 0:
            i = j = 0
        k, state = AL - 2, 0                        # affine: 0 at H, 1 inside F (gap in the ref), 2 inside E
        while True:
            if i < 0 or j < 0 or k < 0:
                break
            lo, hi = windows[i]
            if not lo <= j <= hi:                   # a step out of the band: START
                break
            cell = codes[i][p, j - lo]
            if state == 0:
                if cell == _START:
                    break
                move = cell if not affine else (0 if cell == 0 else None)
                if affine and cell != 0:
                    state = int(cell)
                    continue
            else:
                move = state
            walked[p].append((i, j))
            if move == 0:
                rows[p, 0, k], rows[p, 1, k] = reads[p, i], refs[p, j]
                i, j = i - 1, j - 1
            elif move == 1:
                rows[p, 0, k], rows[p, 1, k] = reads[p, i], ord("-")
                if affine:
                    state = 1 if f_ext[i][p, j - lo] else 0
                i -= 1
            else:
                rows[p, 0, k], rows[p, 1, k] = ord("-"), refs[p, j]
                if affine:
                    state = 2 if e_ext[i][p, j - lo] else 0
                j -= 1
            k -= 1
        idx[p] = (k + 1, AL - 1, k + 1, AL - 1)
    return (rows, idx, walked) if paths else (rows, idx)


def rescore(rows, idx, scoring, affine=False):
    """Score of each gapped alignment (linear or affine gaps; a base pair outside ACGT scores 0)."""
    tab = np.zeros((6, 6), np.int64)
    tab[1:5, 1:5] = scoring.mismatch
    for a in range(1, 5):
        tab[a, a] = scoring.match
    out = np.zeros(len(rows), np.int64)
    for p in range(len(rows)):
        s, e = int(idx[p, 0]), int(idx[p, 1])
        a, b = rows[p, 0, s:e], rows[p, 1, s:e]
        total, prev = 0, None
        for x, y in zip(a.tolist(), b.tolist()):
            kind = "E" if x == ord("-") else ("F" if y == ord("-") else "M")
            if kind == "M":
                total += tab[_CLASS[x], _CLASS[y]]
            elif not affine:
                total += scoring.gap_read if kind == "E" else scoring.gap_ref
            elif kind == "E":
                total += scoring.ext_read if prev == "E" else scoring.open_read
            else:
                total += scoring.ext_ref if prev == "F" else scoring.open_ref
            prev = kind
        out[p] = total
    return out
