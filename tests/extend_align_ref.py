"""Extension alignments (include/valign_hip.h: valign_hip_align_extend_*) restated in numpy / Python, independent of the library:
the matrices X, E, G on int64 cells for both gap models, anchored at the origin -- gap-priced borders, no floor at zero -- filled
anti-diagonal by anti-diagonal for the whole batch at once; the extension record; the end cell under the end-bonus rule; the walk
from there back to the anchor, decided on cell values; the record and the run-length encoded ops.

  scoring: an object with match, mismatch, gap_read, gap_ref, open_read, ext_read, open_ref, ext_ref (hipkernel.Scoring,
  oracle.cpu_ref.Scoring).  Two bases score match / mismatch when both are one of ACGT (either case), anything else scores 0.
  A step along the row (LEFT: a reference base against a gap in the read, op D) costs gap_read (affine: open_read, then ext_read),
  a step down the column (UP: a read base against a gap in the reference, op I) gap_ref (open_ref, then ext_ref).

X[:, i + 1, j + 1] is the definition's X(i, j): index 0 of either axis is the border (-1).  E is the best value that ends in a step
along the row (the horizontal state), G the best that ends in a step down the column (the vertical state); neither exists on a
border.
"""
import numpy as np

_CLASS = np.zeros(256, np.int64)
for _k, _ch in enumerate("ACGT"):
    _CLASS[ord(_ch)] = _CLASS[ord(_ch.lower())] = _k + 1

_NEVER = -(1 << 40)          # a value no maximum takes: a gap state that does not exist on a border

OP_M, OP_I, OP_D, OP_EQ, OP_X = 0, 1, 2, 7, 8
INT32_MAX = 2 ** 31 - 1


def trimmed_lengths(seqs):
    """-> int64 [n]: 1 + the position of the last ACGT byte (either case) of each row, 0 where there is none"""
    good = _CLASS[np.asarray(seqs, np.uint8)] > 0
    n, L = good.shape
    if L == 0:
        return np.zeros(n, np.int64)
    return np.where(good.any(axis=1), L - np.argmax(good[:, ::-1], axis=1), 0).astype(np.int64)


def gap_scores(scoring, affine):
    """-> open_read, ext_read, open_ref, ext_ref: a linear gap is an affine one whose opening costs what an extension does"""
    if affine:
        return int(scoring.open_read), int(scoring.ext_read), int(scoring.open_ref), int(scoring.ext_ref)
    return int(scoring.gap_read), int(scoring.gap_read), int(scoring.gap_ref), int(scoring.gap_ref)


def substitution(reads, refs, scoring):
    """-> S int64 [n, R, F]"""
    rc, fc = _CLASS[np.asarray(reads, np.uint8)], _CLASS[np.asarray(refs, np.uint8)]
    both = (rc[:, :, None] > 0) & (fc[:, None, :] > 0)
    return np.where(both, np.where(rc[:, :, None] == fc[:, None, :], int(scoring.match), int(scoring.mismatch)), 0).astype(np.int64)


def matrices(reads, refs, scoring, affine=False):
    """-> X, E, G int64 [n, R + 1, F + 1] and S int64 [n, R, F]"""
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n, R = reads.shape
    F = refs.shape[1]
    S = substitution(reads, refs, scoring)
    o_r, e_r, o_f, e_f = gap_scores(scoring, affine)
    X = np.zeros((n, R + 1, F + 1), np.int64)
    E = np.full((n, R + 1, F + 1), _NEVER, np.int64)
    G = np.full((n, R + 1, F + 1), _NEVER, np.int64)
    X[:, 0, 1:] = o_r + e_r * np.arange(F)           # the border row: one gap run from the anchor
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
    return X, E, G, S


def extension_record(X, Rp, Fp):
    """ONE pair: X int64 [R + 1, F + 1] -> [score, read_end, ref_end, gscore, gref_end] (the extension scores' record)"""
    if Rp == 0:
        return [0, 0, 0, 0, 0]
    best, bi, bj = 0, 0, 0
    if Fp > 0:
        inside = X[1:Rp + 1, 1:Fp + 1]
        at = int(inside.argmax())                   # row-major: the first cell that holds the maximum
        if inside.flat[at] > 0:
            best, bi, bj = int(inside.flat[at]), at // Fp + 1, at % Fp + 1
    last = X[Rp, :Fp + 1]                            # row Rp - 1, the border column first
    gj = int(last.argmax())                         # the smallest candidate column
    return [best, bi, bj, int(last[gj]), gj]


def end_cell(ext, Rp, end_bonus):
    """The end-bonus rule -> (i, j) of the end cell, 0-based with -1 for a border, or None for the empty alignment"""
    score, read_end, ref_end, gscore, gref_end = ext
    if Rp == 0:
        return None
    if end_bonus >= 0 and gscore + end_bonus >= score:          # (Python integers: no overflow; ties go to the read end)
        return Rp - 1, gref_end - 1
    if score == 0:
        return None
    return read_end - 1, ref_end - 1


def walk(X, E, G, S, i, j, gaps, affine):
    """ONE pair: from cell (i, j) back to the anchor (-1, -1) -> the moves in READING order, each 'M' (DIAG), 'I' (UP) or 'D'
    (LEFT) with the cell it was taken at.  Decided on cell values."""
    o_r, e_r, o_f, e_f = gaps
    moves = []
    state = "H"
    while i >= 0 or j >= 0:
        if j < 0:                                    # the border column: UP, at H
            moves.append(("I", i, j))
            i -= 1
            state = "H"
            continue
        if i < 0:                                    # the border row: LEFT, at H
            moves.append(("D", i, j))
            j -= 1
            state = "H"
            continue
        h = X[i + 1, j + 1]
        if not affine:
            if h == X[i, j] + S[i, j]:
                moves.append(("M", i, j))
                i -= 1
                j -= 1
            elif h == X[i, j + 1] + o_f:
                moves.append(("I", i, j))
                i -= 1
            else:
                assert h == X[i + 1, j] + o_r
                moves.append(("D", i, j))
                j -= 1
            continue
        if state == "H":
            if h == X[i, j] + S[i, j]:
                moves.append(("M", i, j))
                i -= 1
                j -= 1
            elif h == G[i + 1, j + 1]:
                state = "V"                          # nothing is emitted on entering a gap state
            else:
                assert h == E[i + 1, j + 1]
                state = "Z"
        elif state == "V":
            moves.append(("I", i, j))
            if G[i + 1, j + 1] == X[i, j + 1] + o_f:  # opened here (an open wins a tie): back to H
                state = "H"
            i -= 1
        else:
            moves.append(("D", i, j))
            if E[i + 1, j + 1] == X[i + 1, j] + o_r:
                state = "H"
            j -= 1
    moves.reverse()
    return moves


def encode(moves, read, ref, extended):
    """The column rule and the run lengths of the compact result format -> ops [length << 4 | code]"""
    ops = []
    for kind, i, j in moves:
        if kind == "I":
            code = OP_I
        elif kind == "D":
            code = OP_D
        elif not extended:
            code = OP_M
        else:
            code = OP_EQ if (int(read[i]) | 0x20) == (int(ref[j]) | 0x20) else OP_X
        if ops and ops[-1][1] == code:
            ops[-1][0] += 1
        else:
            ops.append([1, code])
    return [(length << 4) | code for length, code in ops]


def rescore(moves, S, gaps):
    """The moves re-scored under the scoring: a maximal run of k gap columns of one kind costs open + (k - 1) * ext"""
    o_r, e_r, o_f, e_f = gaps
    total, prev = 0, None
    for kind, i, j in moves:
        if kind == "M":
            total += int(S[i, j])
        elif kind == "I":
            total += e_f if prev == "I" else o_f
        else:
            total += e_r if prev == "D" else o_r
        prev = kind
    return total


def align(reads, refs, scoring, affine=False, end_bonus=-1, extended=False, chunk=64):
    """-> recs int64 [n, 6] (read_begin, read_end, ref_begin, ref_end, score, n_ops), ops: a list of n lists of uint32 ops,
    ext int64 [n, 5] (the extension records), ends: a list of n end cells ((i, j) or None).  end_bonus may be a tuple of
    bonuses: a list of such results then, one per bonus, from ONE fill of the matrices."""
    if isinstance(end_bonus, (tuple, list)):
        return _align(reads, refs, scoring, affine, tuple(end_bonus), extended, chunk)
    return _align(reads, refs, scoring, affine, (end_bonus,), extended, chunk)[0]


def _align(reads, refs, scoring, affine, bonuses, extended, chunk):
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n = len(reads)
    gaps = gap_scores(scoring, affine)
    Rp_all, Fp_all = trimmed_lengths(reads), trimmed_lengths(refs)
    out = [(np.zeros((n, 6), np.int64), [], np.zeros((n, 5), np.int64), []) for _ in bonuses]
    for b in range(0, n, chunk):
        X, E, G, S = matrices(reads[b:b + chunk], refs[b:b + chunk], scoring, affine)
        for p in range(len(X)):
            g = b + p
            Rp, Fp = int(Rp_all[g]), int(Fp_all[g])
            record = extension_record(X[p], Rp, Fp)
            walked = {}                              # end cell -> (moves' ops, score): bonuses that pick the same cell share the walk
            for (recs, ops, ext, ends), bonus in zip(out, bonuses):
                ext[g] = record
                cell = end_cell(record, Rp, bonus)
                ends.append(cell)
                if cell is None:
                    ops.append([])
                    continue
                if cell not in walked:
                    moves = walk(X[p], E[p], G[p], S[p], cell[0], cell[1], gaps, affine)
                    score = rescore(moves, S[p], gaps)
                    assert score == X[p][cell[0] + 1, cell[1] + 1], (g, score, int(X[p][cell[0] + 1, cell[1] + 1]))
                    walked[cell] = (encode(moves, reads[g], refs[g], extended), score)
                pair_ops, score = walked[cell]
                recs[g] = [0, cell[0] + 1, 0, cell[1] + 1, score, len(pair_ops)]
                ops.append(list(pair_ops))
    return out
