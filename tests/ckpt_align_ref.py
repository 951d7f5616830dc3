"""The checkpointed traceback of long-read alignments (trace_checkpoints = 1), restated in plain numpy / Python with the
strip height as a parameter (a helper of the tests; one pair at a time, small shapes).

The schedule (versalignlib_amd/csrc/ckpt_plan.h): the read's rows are cut into S strips of `strip_rows` rows, the padding
rows above row 0, so strip s holds the read rows i with (i + pad) // strip_rows == s, pad = S * strip_rows - R.
  1. Forward pass: every row is filled, NO pointer is kept; the bottom row of every strip but the last is kept (H with its
     column-0 border; affine gaps: F beside it).  The end cell is found by the reference's rules on the way.
  2. Backward pass, s = S - 1 .. 0: a walk is active in round s when it has not ended and its row lies in strip s.  Strip s is
     filled again from checkpoint row s - 1, columns [0, c] only (c: the walk's current column), this time with pointers; the
     walk crosses it and stops where its row leaves the strip's top, keeping (i, j, k, affine state).  Column 0 of the NW
     variant (j < 0: UP all the way) needs no pointers and is finished in the round where it is reached.
Both passes call ONE row function (_fill_row), as both kernels are instances of one template.

Cell rules, pointers, end cells and the walk are those of oracle/cpu_ref.c (sw_fill / nw_fill / traceback, affine_fill and its
walk): Smith-Waterman and the NW variant, linear and affine gaps, Default tie-breaks.  Results come back in cpu_ref.align's
layout: rows uint8 [n, 2, R + F] right-justified behind zeros, idx int16 [n, 4] = readStart, readEnd, refStart, refEnd.
"""
import numpy as np

SW, NW = 0, 1
NEG_INF = -16384
_START, _DIAG, _UP, _LEFT = 0, 1, 2, 3            # linear pointers; affine H sources: 0 START, 1 DIAG, 2 from F, 3 from E

_CLASS = np.zeros(256, np.int64)
for _c, _v in zip(b"ATCGN", (1, 2, 3, 4, 5)):
    _CLASS[_c] = _v
    _CLASS[ord(chr(_c).lower())] = _v


def _subst(sc):
    tab = np.zeros((6, 6), np.int64)
    tab[1:5, 1:5] = sc.mismatch
    for a in range(1, 5):
        tab[a, a] = sc.match
    return tab


def _top_row(F):
    """The row above read row 0: H = 0 everywhere (index 0 is column -1), F = "minus infinity"."""
    return [0] * (F + 1), [NEG_INF] * (F + 1)


def _fill_row(alg, affine, sc, tab, i, rc, fc, h_up, f_up, cols, want_ptr):
    """Read row i, columns [0, cols), from the row above (h_up / f_up, index j + 1 = column j, index 0 = column -1).
    -> h, f (same layout; entries beyond `cols` are None: never computed) and, with want_ptr, the row's pointers:
    linear a list of codes, affine a list of (source of H, F extended, E extended)."""
    F = len(h_up) - 1
    h = [None] * (F + 1)
    f = [None] * (F + 1)
    ptr = [None] * (F + 1) if want_ptr else None
    srow = tab[rc[i]]
    if not affine:
        gr, gf = sc.gap_read, sc.gap_ref
        h[0] = (i + 1) * gf if alg == NW else 0
        if want_ptr:
            ptr[0] = _UP if alg == NW else _START
        for j in range(cols):
            up, left, diag = h_up[j + 1] + gf, h[j] + gr, h_up[j] + srow[fc[j]]
            v = max(diag, up, left)
            if alg == SW:
                v = max(v, 0)
            h[j + 1] = v
            if want_ptr:
                ptr[j + 1] = _START if (alg == SW and v == 0) else (_DIAG if v == diag else (_UP if v == up else _LEFT))
        return h, f, ptr
    oR, eR, oF, eF = sc.open_read, sc.ext_read, sc.open_ref, sc.ext_ref
    h[0] = oF + i * eF if alg == NW else 0
    f[0] = NEG_INF
    if want_ptr:
        ptr[0] = (2, i > 0, False) if alg == NW else (0, False, False)
    e = NEG_INF
    for j in range(cols):
        e_open, e_extd = h[j] + oR, e + eR
        f_open, f_extd = h_up[j + 1] + oF, f_up[j + 1] + eF
        e = max(e_extd, e_open)
        fv = max(f_extd, f_open)
        diag = h_up[j] + srow[fc[j]]
        v = max(diag, e, fv)
        if alg == SW:
            v = max(v, 0)
        h[j + 1] = v
        f[j + 1] = fv
        if want_ptr:
            src = 0 if (alg == SW and v == 0) else (1 if v == diag else (2 if v == fv else 3))
            ptr[j + 1] = (src, fv != f_open, e != e_open)
    return h, f, ptr


def _forward(alg, affine, sc, tab, rc, fc, strip_rows):
    """-> checkpoints {s: (h, f)} -- the bottom row of every strip but the last -- and the end cell."""
    R, F = len(rc), len(fc)
    S = max(1, -(-R // strip_rows))
    pad = S * strip_rows - R
    h_up, f_up = _top_row(F)
    ckpt = {}
    best, bi, bj = 0, 0, 0
    last_read, last_ref = R - 1, F - 1
    row_arg, snap_arg = 0, -1
    for i in range(R):
        h, f, _ = _fill_row(alg, affine, sc, tab, i, rc, fc, h_up, f_up, F, False)
        if alg == SW:
            for j in range(F):                      # the row-major first strict maximum
                if h[j + 1] > best:
                    best, bi, bj = h[j + 1], i, j
        else:
            if last_read == R - 1 and rc[i] == 0:
                last_read = i - 1
            if last_read + 1 == i:
                snap_arg = row_arg
            row_best, row_arg = h[0], 0
            for j in range(F):
                if last_ref == F - 1 and fc[j] == 0:
                    last_ref = j - 1
                if h[j + 1] > row_best:
                    row_best, row_arg = h[j + 1], j
        h_up, f_up = h, f
        if (i + pad + 1) % strip_rows == 0 and i + 1 < R:
            ckpt[(i + pad) // strip_rows] = (h, f)
    if alg == SW:
        return ckpt, bi, bj
    if snap_arg < 0:
        snap_arg = row_arg
    return ckpt, last_read, min(last_ref, snap_arg)


def align_pair(alg, read, ref, sc, strip_rows, affine=False, stats=None):
    """One pair -> (row_read, row_ref, idx).  `stats` (a dict) counts what the schedule met: rounds, re-filled cells, walks
    that paused inside a vertical gap, that met a horizontal gap at a strip boundary, that finished column 0 above strip 0."""
    read = np.asarray(read, np.uint8)
    ref = np.asarray(ref, np.uint8)
    R, F, AL = len(read), len(ref), len(read) + len(ref)
    rc, fc = _CLASS[read].tolist(), _CLASS[ref].tolist()
    tab = _subst(sc).tolist()
    S = max(1, -(-R // strip_rows))
    pad = S * strip_rows - R
    stats = stats if stats is not None else {}
    for key in ("rounds", "refilled_cells", "paused_in_vertical_gap", "horizontal_gap_at_boundary", "column0_above_strip0", "idle_rounds"):
        stats.setdefault(key, 0)

    ckpt, i, j = _forward(alg, affine, sc, tab, rc, fc, strip_rows)
    row_read, row_ref = np.zeros(AL, np.uint8), np.zeros(AL, np.uint8)
    k, state, done = AL - 2, 0, False              # affine state: 0 at H, 2 inside F (gap in the ref), 3 inside E
    strip_of = lambda row: 0 if row < 0 else (row + pad) // strip_rows
    last_move = prev_move = None

    def emit(a, b):
        nonlocal k
        row_read[k], row_ref[k] = a, b
        k -= 1

    for s in range(S - 1, -1, -1):
        if done or strip_of(i) != s:
            stats["idle_rounds"] += 1
            continue
        stats["rounds"] += 1
        lo, hi = max(s * strip_rows - pad, 0), min((s + 1) * strip_rows - pad, R) - 1
        # ---- re-fill strip s, columns [0, j], from checkpoint row s - 1 ----
        h_up, f_up = ckpt[s - 1] if s > 0 else _top_row(F)
        ptrs = {}
        for r in range(lo, hi + 1):
            h_up, f_up, ptrs[r] = _fill_row(alg, affine, sc, tab, r, rc, fc, h_up, f_up, j + 1, True)
            stats["refilled_cells"] += j + 1
        # ---- walk strip s ----
        resumed = True
        while True:
            if i < 0:                               # row 0: START
                done = True
                break
            if j < 0:                               # column 0: SW START; NW variant UP all the way, no pointers needed
                if alg == NW:
                    if lo > 0:
                        stats["column0_above_strip0"] += 1
                    while i >= 0:
                        emit(read[i], ord("-"))
                        i -= 1
                done = True
                break
            if i < lo:                              # the next cell lies in the strip above: the next round's
                if state == 2 or (not affine and last_move == _UP):
                    stats["paused_in_vertical_gap"] += 1
                if prev_move == _LEFT:              # (the strip's top row ended a horizontal gap right before the crossing)
                    stats["horizontal_gap_at_boundary"] += 1
                break
            q = ptrs[i][j + 1]
            if not affine:
                if q == _START:
                    done = True
                    break
                move = q
            elif state == 0:
                if q[0] == 0:
                    done = True
                    break
                if q[0] != 1:
                    state = q[0]                    # enter the gap state, nothing emitted yet
                    continue
                move = _DIAG
            elif state == 2:
                move = _UP
                state = 2 if q[1] else 0
            else:
                move = _LEFT
                state = 3 if q[2] else 0
            if resumed and s < S - 1 and move == _LEFT:      # (the walk resumes inside a horizontal gap of the strip's bottom row)
                stats["horizontal_gap_at_boundary"] += 1
            resumed = False
            prev_move, last_move = last_move, move
            if k < 0:
                done = True
                break
            if move == _DIAG:
                emit(read[i], ref[j])
                i, j = i - 1, j - 1
            elif move == _UP:
                emit(read[i], ord("-"))
                i -= 1
            else:
                emit(ord("-"), ref[j])
                j -= 1
    return row_read, row_ref, np.array([k + 1, AL - 1, k + 1, AL - 1], np.int16)


def align(alg, reads, refs, sc, strip_rows, affine=False, stats=None):
    """-> rows uint8 [n, 2, R + F], idx int16 [n, 4] of the batch, pair by pair."""
    reads = np.ascontiguousarray(reads, np.uint8)
    refs = np.ascontiguousarray(refs, np.uint8)
    n, AL = len(reads), reads.shape[1] + refs.shape[1]
    rows = np.zeros((n, 2, AL), np.uint8)
    idx = np.zeros((n, 4), np.int16)
    for p in range(n):
        rows[p, 0], rows[p, 1], idx[p] = align_pair(alg, reads[p], refs[p], sc, strip_rows, affine, stats)
    return rows, idx
