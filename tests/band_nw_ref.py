"""The banded NW variant (band_nw = 1), restated in numpy (a helper of the tests, vectorised over pairs).

Definition (include/valign_hip.h, valign_hip_set_band_nw): the reference's Needleman-Wunsch variant (oracle/cpu_ref.c
nw_score_one / nw_fill, cpu_ref_fills.inc affine_fill with alg = 1) on int64 cells, on the block band of band_width
(band_align_ref.row_window = oracle/cpu_ref.c band_columns with block_rows / col_align):
  * a cell outside its row's window [lo_i, hi_i] is ABSENT (minus infinity; affine: H, E and F): never a candidate, never part
    of a maximum or an arg-max;
  * the border row above row 0 is present at every column (0, START); the border column left of column 0 is present at row i
    only where lo_i == 0 -- scores: 0; alignments: (i + 1) * gap_ref, UP (linear), open_ref + i * ext_ref, from F (affine);
  * present cells: the unbanded recurrence and tie-breaks -- DIAG > UP > LEFT; affine: DIAG > F > E, open preferred on ties;
  * score = max(0, present cells of the last row, present cells of the last column);
  * end cell: end_i the last row before the first invalid read byte, end_j = min(last_ref, arg), arg the first strict arg-max
    over the present cells of row end_i, the running best starting at the border column's value where lo == 0, else at absent;
    an absent start cell gives the empty alignment (all-zero rows, four coordinates R + F - 1);
  * bands with 2 * (band_width / 2) + 1 < ceil(F / R) are refused (ValueError): consecutive blocks' windows would not connect.
Rows and coordinates come back in cpu_ref.align's layout.
"""
import numpy as np

from band_align_ref import _CLASS, _scores, row_window

ABSENT = -(1 << 40)


def check_connects(R, F, band_width):
    if 2 * (band_width // 2) + 1 < -(-F // R):
        raise ValueError("band_nw: band_width %d is too narrow for %d x %d (windows do not connect)" % (band_width, R, F))


def _row(i, lo, hi, h_prev, f_prev, left, sub, sc, affine):
    """One row's window.  h_prev / f_prev: [n, F + 1], index j + 1 = column j, index 0 = the border column; left: [n] the
    row's own border-column value (ABSENT where lo > 0).  -> h, f, code (and, affine, e_ext / f_ext) over [lo, hi]."""
    js = np.arange(lo, hi + 1)
    d = h_prev[:, lo:hi + 1] + sub
    up = h_prev[:, lo + 1:hi + 2]
    if not affine:
        u = up + sc.gap_ref
        a = np.maximum(d, u)
        gr = sc.gap_read
        # H[j] = max(A[j], H[j - 1] + gap_read), H[lo - 1] = left: a running maximum
        x = np.concatenate([(left - (lo - 1) * gr)[:, None], a - js * gr], axis=1)
        h = np.maximum.accumulate(x, axis=1)[:, 1:] + js * gr
        code = np.where(h == d, 0, np.where(h == u, 1, 2))
        return h, None, code, None, None
    oR, eR, oF, eF = sc.open_read, sc.ext_read, sc.open_ref, sc.ext_ref
    f_open = up + oF
    f_extd = f_prev[:, lo + 1:hi + 2] + eF
    f = np.maximum(f_open, f_extd)
    b = np.maximum(d, f)
    # E[j] = max(E[j - 1] + ext_read, H[j - 1] + open_read), H = max(B, E), E[lo - 1] absent, H[lo - 1] = left:
    # E[j] = max(E[j - 1] + max(ext, open), B[j - 1] + open)
    c = max(eR, oR)
    x = np.empty_like(b)
    x[:, 0] = left + oR
    x[:, 1:] = b[:, :-1] + oR
    e = np.maximum.accumulate(x - js * c, axis=1) + js * c
    h = np.maximum(b, e)
    h_left = np.concatenate([left[:, None], h[:, :-1]], axis=1)
    e_left = np.concatenate([np.full((len(left), 1), ABSENT, np.int64), e[:, :-1]], axis=1)
    code = np.where(h == d, 0, np.where(h == f, 1, 2))
    return h, f, code, (e_left + eR) > (h_left + oR), f_extd > f_open


def _floor_absent(v):
    return np.maximum(v, ABSENT)            # (absent plus a score is still absent: no drift over a long matrix)


def score_banded_nw(reads, refs, band_width, scoring, block_rows=1, col_align=1, affine=False):
    """-> int64 [n]: the banded NW-variant scores (module docstring).  band_width 0: every cell."""
    reads = np.ascontiguousarray(reads, np.uint8)
    refs = np.ascontiguousarray(refs, np.uint8)
    n, R = reads.shape
    F = refs.shape[1]
    if band_width > 0:
        check_connects(R, F, band_width)
    tab, rc, fc = _scores(scoring, reads, refs)
    h_prev = np.zeros((n, F + 1), np.int64)                  # the border row
    f_prev = np.full((n, F + 1), ABSENT, np.int64)
    best = np.zeros(n, np.int64)
    for i in range(R):
        lo, hi = row_window(i, R, F, band_width, block_rows, col_align) if band_width > 0 else (0, F - 1)
        left = np.full(n, 0 if lo == 0 else ABSENT, np.int64)
        h, f, _, _, _ = _row(i, lo, hi, h_prev, f_prev, left, tab[rc[:, i:i + 1], fc[:, lo:hi + 1]], scoring, affine)
        h = _floor_absent(h)
        if hi == F - 1:
            best = np.maximum(best, h[:, -1])
        if i == R - 1:
            best = np.maximum(best, h.max(axis=1))
        h_prev = np.full((n, F + 1), ABSENT, np.int64)
        h_prev[:, lo + 1:hi + 2] = h
        if lo == 0:
            h_prev[:, 0] = 0
        if affine:
            f_prev = np.full((n, F + 1), ABSENT, np.int64)
            f_prev[:, lo + 1:hi + 2] = _floor_absent(f)
    return best


def align_banded_nw(reads, refs, band_width, scoring, block_rows=1, col_align=1, affine=False):
    """-> rows uint8 [n, 2, R + F], idx int16 [n, 4] of the banded NW-variant alignments (module docstring)."""
    reads = np.ascontiguousarray(reads, np.uint8)
    refs = np.ascontiguousarray(refs, np.uint8)
    n, R = reads.shape
    F = refs.shape[1]
    if band_width > 0:
        check_connects(R, F, band_width)
    tab, rc, fc = _scores(scoring, reads, refs)
    h_prev = np.zeros((n, F + 1), np.int64)
    f_prev = np.full((n, F + 1), ABSENT, np.int64)
    windows, codes, e_exts, f_exts, args = [], [], [], [], []
    for i in range(R):
        lo, hi = row_window(i, R, F, band_width, block_rows, col_align) if band_width > 0 else (0, F - 1)
        border = (scoring.open_ref + i * scoring.ext_ref) if affine else (i + 1) * scoring.gap_ref
        left = np.full(n, border if lo == 0 else ABSENT, np.int64)
        h, f, code, e_ext, f_ext = _row(i, lo, hi, h_prev, f_prev, left, tab[rc[:, i:i + 1], fc[:, lo:hi + 1]], scoring, affine)
        h = _floor_absent(h)
        # first strict arg-max of the row, the running best starting at the border column (column 0 when it wins)
        rmax = h.max(axis=1)
        args.append(np.where(rmax > left, lo + h.argmax(axis=1), 0))
        windows.append((lo, hi))
        codes.append(code.astype(np.uint8))
        e_exts.append(e_ext)
        f_exts.append(f_ext)
        h_prev = np.full((n, F + 1), ABSENT, np.int64)
        h_prev[:, lo + 1:hi + 2] = h
        h_prev[:, 0] = left
        if affine:
            f_prev = np.full((n, F + 1), ABSENT, np.int64)
            f_prev[:, lo + 1:hi + 2] = _floor_absent(f)
    AL = R + F
    rows = np.zeros((n, 2, AL), np.uint8)
    idx = np.zeros((n, 4), np.int16)
    bad_read = _CLASS[reads] == 0
    bad_ref = _CLASS[refs] == 0
    for p in range(n):
        i = int(np.argmax(bad_read[p])) - 1 if bad_read[p].any() else R - 1
        last_ref = int(np.argmax(bad_ref[p])) - 1 if bad_ref[p].any() else F - 1
        j = min(last_ref, int(args[i][p])) if i >= 0 else min(last_ref, 0)
        k, state = AL - 2, 0                        # affine: 0 at H, 1 inside F (gap in the ref), 2 inside E
        if i >= 0:
            lo, hi = windows[i]
            if not (lo <= j <= hi or (j == -1 and lo == 0)):
                i = -1                              # the start cell is absent: the empty alignment
        while i >= 0 and k >= 0:
            lo, hi = windows[i]
            if j < 0:                               # the border column: UP to the border row
                assert lo == 0
                rows[p, 0, k], rows[p, 1, k] = reads[p, i], ord("-")
                i, k, state = i - 1, k - 1, 0
                continue
            assert lo <= j <= hi, "a pointer led out of the band"
            if state == 0:
                move = int(codes[i][p, j - lo])
                if affine and move != 0:
                    state = move
                    continue
            else:
                move = state
            if move == 0:
                rows[p, 0, k], rows[p, 1, k] = reads[p, i], refs[p, j]
                i, j = i - 1, j - 1
            elif move == 1:
                rows[p, 0, k], rows[p, 1, k] = reads[p, i], ord("-")
                if affine:
                    state = 1 if f_exts[i][p, j - lo] else 0
                i -= 1
            else:
                rows[p, 0, k], rows[p, 1, k] = ord("-"), refs[p, j]
                if affine:
                    state = 2 if e_exts[i][p, j - lo] else 0
                j -= 1
            k -= 1
        idx[p] = (k + 1, AL - 1, k + 1, AL - 1)
    return rows, idx
