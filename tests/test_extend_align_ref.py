"""tests/extend_align_ref.py against itself and against tests/extend_ref.py: its extension records are the extension scores'
reference's; on every shape up to 5 x 5 the walked alignment re-scores to X(end cell), which is the maximum over ALL anchor-to-cell
paths, enumerated one by one with maximal gap runs priced open + (k - 1) * ext; hand-written tie cases pin the priorities.  No GPU."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

import extend_align_ref as ref
import extend_ref

LETTERS = np.frombuffer(b"ACGN", np.uint8)


def _sc(match, mismatch, gap_read, gap_ref, *affine):
    o_r, e_r, o_f, e_f = affine if affine else (gap_read, gap_read, gap_ref, gap_ref)
    return SimpleNamespace(match=match, mismatch=mismatch, gap_read=gap_read, gap_ref=gap_ref, open_read=o_r, ext_read=e_r, open_ref=o_f, ext_ref=e_f)


# one linear scoring, two affine ones: four different scores, and open == ext (every extension ties with an open)
SCORINGS = {"linear": (_sc(2, -1, -2, -4), False), "affine": (_sc(2, -1, -3, -3, -6, -2, -4, -1), True),
            "affine open == ext": (_sc(2, -1, -3, -3, -2, -2, -1, -1), True)}


def _ops_text(ops):
    return "".join("%d%s" % (op >> 4, {0: "M", 1: "I", 2: "D", 7: "=", 8: "X"}[op & 15]) for op in ops)


def _consumed(ops):
    read = sum(op >> 4 for op in ops if (op & 15) in (0, 1, 7, 8))
    refc = sum(op >> 4 for op in ops if (op & 15) in (0, 2, 7, 8))
    return read, refc


def _best_by_enumeration(S, gaps):
    """Every DIAG / UP / LEFT path from the anchor, one by one -> best[i + 1][j + 1]: the best score of a path that ends in cell
    (i, j), borders included"""
    o_r, e_r, o_f, e_f = gaps
    R, F = S.shape
    best = [[None] * (F + 1) for _ in range(R + 1)]

    def go(i, j, score, prev):
        if best[i + 1][j + 1] is None or score > best[i + 1][j + 1]:
            best[i + 1][j + 1] = score
        if i + 1 < R and j + 1 < F:
            go(i + 1, j + 1, score + int(S[i + 1, j + 1]), "M")
        if i + 1 < R:
            go(i + 1, j, score + (e_f if prev == "I" else o_f), "I")
        if j + 1 < F:
            go(i, j + 1, score + (e_r if prev == "D" else o_r), "D")

    go(-1, -1, 0, None)
    return best


def _sequences(rng, L, cap):
    """every sequence of length L over the alphabet where there are at most `cap`, else `cap` random ones"""
    if 4 ** L <= cap:
        return np.array(list(itertools.product(LETTERS, repeat=L)), np.uint8).reshape(-1, L)
    return LETTERS[rng.integers(0, 4, (cap, L))]


@pytest.mark.parametrize("name", list(SCORINGS))
def test_extension_records_equal_the_extension_reference(name):
    sc, affine = SCORINGS[name]
    rng = np.random.default_rng(5)
    for R, F in ((1, 1), (3, 7), (12, 20), (33, 17)):
        reads, refs = LETTERS[rng.integers(0, 4, (40, R))], LETTERS[rng.integers(0, 4, (40, F))]
        refs[::2, :min(R, F)] = reads[::2, :min(R, F)]
        reads[::3, R // 2:] = ord("N")
        refs[1::4, F // 2:] = 0
        for bonus in (-1, 0, 7):
            recs, ops, ext, ends = ref.align(reads, refs, sc, affine, end_bonus=bonus)
            assert (ext == extend_ref.extend(reads, refs, sc, affine)).all(), (name, R, F, bonus)


@pytest.mark.parametrize("name", list(SCORINGS))
def test_walk_rescores_to_the_end_cell_and_that_is_the_best_path(name):
    sc, affine = SCORINGS[name]
    gaps = ref.gap_scores(sc, affine)
    rng = np.random.default_rng(17)
    kinds = {"best": 0, "read end": 0, "border column": 0, "empty": 0}
    for R in range(1, 6):
        for F in range(1, 6):
            rd = _sequences(rng, R, 16)
            rf = _sequences(rng, F, 16)
            pick = rng.permutation(len(rd) * len(rf))[:40]
            reads, refs = rd[pick // len(rf)], rf[pick % len(rf)]
            X, E, G, S = ref.matrices(reads, refs, sc, affine)
            best = [_best_by_enumeration(S[p], gaps) for p in range(len(reads))]
            for p in range(len(reads)):
                assert (np.array(best[p], np.int64) == X[p]).all(), (name, reads[p].tobytes(), refs[p].tobytes())
            for bonus in (-1, 0, 3, ref.INT32_MAX):
                for extended in (False, True):
                    recs, ops, ext, ends = ref.align(reads, refs, sc, affine, end_bonus=bonus, extended=extended)
                    for p in range(len(reads)):
                        what = (name, reads[p].tobytes(), refs[p].tobytes(), bonus)
                        if ends[p] is None:
                            assert recs[p].tolist() == [0] * 6 and ops[p] == [], what
                            assert ref.trimmed_lengths(reads[p:p + 1])[0] == 0 or (ext[p, 0] == 0 and (bonus < 0 or ext[p, 3] + bonus < 0)), what
                            kinds["empty"] += 1
                            continue
                        i, j = ends[p]
                        assert recs[p, 0] == 0 and recs[p, 2] == 0 and recs[p, 1] == i + 1 and recs[p, 3] == j + 1, what
                        assert recs[p, 4] == X[p, i + 1, j + 1] == best[p][i + 1][j + 1], what
                        assert recs[p, 4] == (ext[p, 3] if (i + 1, j + 1) == (ref.trimmed_lengths(reads[p:p + 1])[0], ext[p, 4]) and bonus >= 0 and
                                              ext[p, 3] + bonus >= ext[p, 0] else ext[p, 0]), what
                        assert _consumed(ops[p]) == (i + 1, j + 1) and recs[p, 5] == len(ops[p]), what
                        codes = {op & 15 for op in ops[p]}
                        assert codes <= ({1, 2, 7, 8} if extended else {0, 1, 2}), what
                        assert all((a & 15) != (b & 15) for a, b in zip(ops[p], ops[p][1:])), what          # runs are maximal
                        kinds["border column" if j < 0 else ("read end" if bonus >= 0 and ext[p, 3] + bonus >= ext[p, 0] else "best")] += 1
    assert min(kinds.values()) > 50, kinds


def _one(read, refseq, sc, affine, bonus=-1, extended=False):
    reads = np.frombuffer(read, np.uint8)[None, :]
    refs = np.frombuffer(refseq, np.uint8)[None, :]
    recs, ops, ext, ends = ref.align(reads, refs, sc, affine, end_bonus=bonus, extended=extended)
    return _ops_text(ops[0]), recs[0].tolist(), ext[0].tolist()


def test_linear_ties_diag_over_up_over_left():
    # X(0,0) of A / C: diagonal -2, from above X(-1,0) + gap_ref = -2, from the left X(0,-1) + gap_read = -2 -- all three tie, and
    # the match behind it makes (1,1) the best cell: the walk passes (0,0) and takes DIAG
    assert _one(b"AG", b"CG", _sc(5, -2, -1, -1), False) == ("2M", [0, 2, 0, 2, 3, 1], [3, 2, 2, 3, 2])
    # mismatch -3: DIAG loses, UP and LEFT tie at -2.  UP: a read base against a gap at (0,0), then LEFT along the border row --
    # in reading order D, I, M (LEFT first would read I, D, M)
    assert _one(b"AG", b"CG", _sc(5, -3, -1, -1), False) == ("1D1I1M", [0, 2, 0, 2, 3, 3], [3, 2, 2, 3, 2])
    # AA / A: X(1,0) is 0 by DIAG from the border column (X(0,-1) + 1) and by UP from X(0,0) = 1: DIAG, so the gap is the border's
    assert _one(b"AA", b"A", _sc(1, -1, -1, -1), False, bonus=ref.INT32_MAX) == ("1I1M", [0, 2, 0, 1, 0, 2], [1, 1, 1, 0, 1])
    # ... and '=' / X, a first op I
    assert _one(b"AA", b"A", _sc(1, -1, -1, -1), False, bonus=ref.INT32_MAX, extended=True)[0] == "1I1="


def test_read_end_on_the_border_column_and_empty():
    sc = _sc(2, -1, -2, -4)
    # no reference base: the read end is the border column, the ops are Rp I, ref_end = 0
    text, rec, ext = _one(b"ACG", b"NN", sc, False, bonus=100)
    assert (text, rec, ext) == ("3I", [0, 3, 0, 0, -12, 1], [0, 0, 0, -12, 0])
    # the same pair without a bonus: score 0, empty
    assert _one(b"ACG", b"NN", sc, False) == ("", [0] * 6, [0, 0, 0, -12, 0])
    # a bonus too small for the read end keeps the best cell; ties go to the read end
    text, rec, ext = _one(b"ACT", b"ACG", sc, False, bonus=0)
    assert ext == [4, 2, 2, 3, 3] and (text, rec) == ("2M", [0, 2, 0, 2, 4, 1])
    assert _one(b"ACT", b"ACG", sc, False, bonus=1)[:2] == ("3M", [0, 3, 0, 3, 3, 1])
    # a read of only N
    assert _one(b"NN", b"AC", sc, False, bonus=ref.INT32_MAX) == ("", [0] * 6, [0] * 5)


def test_affine_open_wins_a_tie_with_an_extension():
    # open == ext in both directions: every extension of a gap state ties with an opening from H.  AAC / A, walked from the read
    # end (2,0): the diagonal loses there (C against A), so the walk enters the vertical state; G(2,0) = X(1,0) + open = G(1,0) + ext,
    # the open wins, the walk is back at H in (1,0) -- and takes DIAG from the border column there (X(1,0) = X(0,-1) + 1), where an
    # extension would have stayed in the state and walked UP: 1I 1M 1I, not 1M 2I
    sc = _sc(1, -3, -1, -1, -1, -1, -1, -1)
    text, rec, ext = _one(b"AAC", b"A", sc, True, bonus=ref.INT32_MAX)
    assert rec[:4] == [0, 3, 0, 1] and rec[4] == ext[3]
    assert text == "1I1M1I"
    # the linear rule on the same scores walks the same path
    assert _one(b"AAC", b"A", _sc(1, -3, -1, -1), False, bonus=ref.INT32_MAX)[0] == "1I1M1I"
    # four different scores, extension cheaper than opening: a gap of two is ONE run (open + ext), walked inside the state
    sc = _sc(2, -3, -3, -3, -4, -1, -4, -1)
    assert _one(b"ACGTAC", b"ACAC", sc, True, bonus=ref.INT32_MAX)[:2] == ("2M2I2M", [0, 6, 0, 4, 3, 3])
    assert _one(b"ACAC", b"ACGTAC", sc, True, bonus=ref.INT32_MAX)[:2] == ("2M2D2M", [0, 4, 0, 6, 3, 3])
