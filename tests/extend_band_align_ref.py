"""Banded extension alignments (include/valign_hip.h: valign_hip_set_extend_band_align) restated in numpy / Python, independent of
the library: the matrices X, E, G of extension alignments on int64 cells with the cells outside the band ABSENT -- a value no
maximum takes and no cell equals -- filled anti-diagonal by anti-diagonal; the banded extension record; the end cell under the
end-bonus rule; the walk from there back to the anchor, decided on cell values; the record and the run-length encoded ops.

  band: w = band_width // 2; rows in blocks of B consecutive read positions counted from row 0 (the library: B = 8; B = 1 is the
  per-cell band |i - j| <= w).  Cell (i, j), 0 <= i < R, -1 <= j < F, is present iff B * (i // B) - w <= j <= B * (i // B) + B - 1
  + w; cell (-1, j) iff j + 1 <= w.  Present border cells hold the unbanded closed forms.
  end cell: the rule of extension alignments in Python integers.  An unreached read end (gscore = UNREACHED) is never chosen:
  UNREACHED + INT32_MAX = -1 < 0 <= score.

X[:, i + 1, j + 1] is the definition's X(i, j): index 0 of either axis is the border (-1).  Which cells are present and when a read
end is unreached are extend_band_ref's statements; the walk, the encoder, the re-scoring and the end-bonus rule are
extend_align_ref's -- they read cell values only, and an absent value equals none.
"""
import numpy as np

from extend_align_ref import INT32_MAX, encode, end_cell, gap_scores, rescore, substitution, trimmed_lengths, walk  # noqa: F401
from extend_band_ref import BLOCK_ROWS, UNREACHED, present, unreached  # noqa: F401

_NEVER = -(1 << 40)             # an absent cell, and a gap state that does not exist
_LOST = _NEVER // 2             # anything below derives from an absent value


def matrices(reads, refs, scoring, band_width, affine=False, B=BLOCK_ROWS):
    """-> X, E, G int64 [n, R + 1, F + 1], S int64 [n, R, F], P bool [R + 1, F + 1] (the present cells).  Absent cells and gap
    states without a present source hold _NEVER."""
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n, R = reads.shape
    F = refs.shape[1]
    P = present(R, F, band_width, B)
    S = substitution(reads, refs, scoring)
    o_r, e_r, o_f, e_f = gap_scores(scoring, affine)
    X = np.full((n, R + 1, F + 1), _NEVER, np.int64)
    E = np.full((n, R + 1, F + 1), _NEVER, np.int64)
    G = np.full((n, R + 1, F + 1), _NEVER, np.int64)
    X[:, 0, 0] = 0
    X[:, 0, 1:] = np.where(P[0, 1:], o_r + e_r * np.arange(F), _NEVER)          # the border row: one gap run from the anchor
    X[:, 1:, 0] = np.where(P[1:, 0], o_f + e_f * np.arange(R), _NEVER)[None, :]
    for d in range(2, R + F + 1):
        i = np.arange(max(1, d - F), min(R, d - 1) + 1)
        j = d - i
        keep = P[i, j]
        i, j = i[keep], j[keep]
        if i.size == 0:
            continue
        diag = X[:, i - 1, j - 1] + S[:, i - 1, j - 1]
        e = np.maximum(E[:, i, j - 1] + e_r, X[:, i, j - 1] + o_r)
        g = np.maximum(G[:, i - 1, j] + e_f, X[:, i - 1, j] + o_f)
        x = np.maximum(diag, np.maximum(e, g))
        assert (x > _LOST).all(), "a present cell without a present candidate"
        E[:, i, j] = np.where(e > _LOST, e, _NEVER)         # (an absent source stays absent: nothing drifts)
        G[:, i, j] = np.where(g > _LOST, g, _NEVER)
        X[:, i, j] = x
    return X, E, G, S, P


def extension_record(X, P, Rp, Fp):
    """ONE pair: X int64 [R + 1, F + 1], P the present cells -> [score, read_end, ref_end, gscore, gref_end] under the band"""
    if Rp == 0:
        return [0, 0, 0, 0, 0]
    best, bi, bj = 0, 0, 0
    if Fp > 0:
        inside = np.where(P[1:Rp + 1, 1:Fp + 1], X[1:Rp + 1, 1:Fp + 1], _NEVER)
        at = int(inside.argmax())                   # row-major: the first cell that holds the maximum
        if inside.flat[at] > 0:
            best, bi, bj = int(inside.flat[at]), at // Fp + 1, at % Fp + 1
    cand = P[Rp, :Fp + 1]                            # row Rp - 1, the border column first
    if not cand.any():
        return [best, bi, bj, UNREACHED, 0]
    last = np.where(cand, X[Rp, :Fp + 1], _NEVER)
    gj = int(last.argmax())                         # the smallest candidate column
    return [best, bi, bj, int(last[gj]), gj]


def align(reads, refs, scoring, band_width, affine=False, end_bonus=-1, extended=False, B=BLOCK_ROWS, chunk=16):
    """-> recs int64 [n, 6] (read_begin, read_end, ref_begin, ref_end, score, n_ops), ops: a list of n lists of uint32 ops,
    ext int64 [n, 5] (the banded extension records), ends: a list of n end cells ((i, j) or None), paths: a list of n lists of
    the moves (kind, i, j) in reading order.  end_bonus may be a tuple of bonuses: a list of such results then, one per bonus,
    from ONE fill of the matrices."""
    many = isinstance(end_bonus, (tuple, list))
    bonuses = tuple(end_bonus) if many else (end_bonus,)
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    n = len(reads)
    gaps = gap_scores(scoring, affine)
    Rp_all, Fp_all = trimmed_lengths(reads), trimmed_lengths(refs)
    out = [(np.zeros((n, 6), np.int64), [], np.zeros((n, 5), np.int64), [], []) for _ in bonuses]
    for b in range(0, n, chunk):
        X, E, G, S, P = matrices(reads[b:b + chunk], refs[b:b + chunk], scoring, band_width, affine, B)
        for p in range(len(X)):
            g = b + p
            Rp, Fp = int(Rp_all[g]), int(Fp_all[g])
            record = extension_record(X[p], P, Rp, Fp)
            assert (record[3] == UNREACHED) == unreached(Rp, Fp, band_width, B), (g, record)
            walked = {}                              # end cell -> (moves, ops, score): bonuses that pick the same cell share the walk
            for (recs, ops, ext, ends, paths), bonus in zip(out, bonuses):
                ext[g] = record
                cell = end_cell(record, Rp, bonus)
                ends.append(cell)
                if cell is None:
                    ops.append([])
                    paths.append([])
                    continue
                assert P[cell[0] + 1, cell[1] + 1], (g, cell, "an absent end cell")
                if cell not in walked:
                    moves = walk(X[p], E[p], G[p], S[p], cell[0], cell[1], gaps, affine)
                    score = rescore(moves, S[p], gaps)
                    assert score == X[p][cell[0] + 1, cell[1] + 1], (g, score, int(X[p][cell[0] + 1, cell[1] + 1]))
                    walked[cell] = (moves, encode(moves, reads[g], refs[g], extended), score)
                moves, pair_ops, score = walked[cell]
                recs[g] = [0, cell[0] + 1, 0, cell[1] + 1, score, len(pair_ops)]
                ops.append(list(pair_ops))
                paths.append(moves)
    return out if many else out[0]
