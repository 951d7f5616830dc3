"""The tilted biased int16 Smith-Waterman sweep with symmetric affine gaps taking its substitution scores from ROW TABLES, as
score_kernel runs it (dp_kernels.hip.h: wave_setup_tables, the step's kRowTables / kRowTablesRepair forms), restated on the CPU
(no GPU, no HIP code involved).  tests/test_sym_affine_inframe_sweep.py restates the sweep with the LDS profile; this file keeps
its cell, hand-over, accumulators and rotation and changes where S' comes from:

  * each row of a lane holds four bytes per pair, the row's read base against reference classes 1 .. 4: match' = match + 2x or
    mismatch' = mismatch + 2x, all four zero' = 2x where the row is a padding row or the base no ACGT, row 0 of every lane plus
    o - x.  Every byte is asserted to be one (cell_rules.h: sym_affine_row_tables_ok);
  * a column selects one of them by its reference base.  A base that is no ACGT, and every column outside [0, len(ref)),
    selects the constant 0 -- NOT zero' -- which is what this file is about:
      - left of column 0 every cell stays exactly at its floor (asserted cell by cell);
      - right of the reference's last ACGT column no diagonal candidate exceeds what the columns before it offered (asserted);
      - every operand of every maximum stays in [0x0400, 0x7BFF] (the imported maxima assert it), down to B + x and B - (o - x),
        at the rule's byte edges and at the tilted window's upper edge;
  * a base that is no ACGT BEFORE the reference's last ACGT base must score zero': such a pair runs the repairing form, which
    sets every half that selected 0 to zero' (row 0: + o - x), pads included.  The plain form is shown to be WRONG there.

`cols` sweeps further columns than the reference has ACGT bases: a pair whose neighbours in the wave have longer references.
Scores are compared exactly with oracle.cpu_ref.score."""
import sys

import numpy as np
import pytest

import test_sym_affine_tilted_sweep as frame
from test_sym_affine_tilted_sweep import GAPS, SUBS, WINDOW, _CLASS, _add16, _i16, _oracle, _related, tilt_bias, tilt_top_index

TABLES, REPAIR = "row_tables", "row_tables_repair"


def _hmax(*patterns):
    return frame._hmax(*patterns)


def rule_ok(match, mismatch, gap_open, gap_ext):
    """cell_rules.h: sym_affine_row_tables_ok, the part about the bytes"""
    o, x = -gap_open, -gap_ext
    return o - x >= 0 and min(match, mismatch, 0) + 2 * x >= 0 and max(match, mismatch, 0) + 2 * x + (o - x) <= 255


def last_acgt_end(ref):
    cols = [j for j, b in enumerate(ref) if 1 <= _CLASS.get(int(b), 0) <= 4]
    return cols[-1] + 1 if cols else 0


def needs_repair(ref):
    return any(not 1 <= _CLASS.get(int(b), 0) <= 4 for b in ref[:last_acgt_end(ref)])


def sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K, form, cols=None):
    R = len(read)
    rows = G * K
    assert R <= rows and K % 2 == 0 and rule_ok(match, mismatch, gap_open, gap_ext)
    o, x = -gap_open, -gap_ext
    ox = o - x
    B = tilt_bias(match, mismatch, gap_open, gap_ext)
    end = last_acgt_end(ref)
    F = end if cols is None else cols                               # the wave's cols_used
    assert F >= end
    # the row tables
    T = []
    for p in range(rows):
        a = _CLASS.get(int(read[p - (rows - R)]), 0) if p >= rows - R else 0
        row = [(match if a == c else mismatch) + 2 * x if 1 <= a <= 4 else 2 * x for c in (1, 2, 3, 4)]
        row = [v + (ox if p % K == 0 else 0) for v in row]
        assert all(0 <= v <= 255 for v in row), row
        T.append(row)
    # the selector stream: a table byte, or None for the constant 0
    sel = [(_CLASS.get(int(ref[j]), 0) - 1 if 1 <= _CLASS.get(int(ref[j]), 0) <= 4 else None) if j < len(ref) else None for j in range(F)]
    lead = (rows - R) // K if rows > R else 0
    steps = F + G - 1 - lead

    def u_of(l, q, t):
        return l * (K - 1) + q + t + 2

    def score(l, q, j):
        c = sel[j] if 0 <= j < F else None
        if c is not None:
            return T[l * K + q][c]
        return 2 * x + (ox if q == 0 else 0) if form == REPAIR else 0

    Hl = [[_add16(B, x * u_of(l, q, -1)) for q in range(K)] for l in range(G)]
    El = [list(row) for row in Hl]
    HOl = [[_add16(v, -ox) for v in row] for row in Hl]
    up0 = [_add16(B, x * u_of(l, -1, -1) - ox) for l in range(G)]
    f_last = [HOl[l][K - 1] for l in range(G)]
    s0 = K - steps % K
    fl = [[_add16(B, x * u_of(l, (i - s0) % K, 0)) for i in range(K)] for l in range(G)]
    acc = [list(row) for row in fl]
    dprev = [[_add16(B, x * u_of(l, q - 1, 0)) if q & 1 else None for q in range(K)] for l in range(G)]
    lead_border = [_add16(B, x * u_of(0, -1, 0) - ox)]
    offered = [0]                                                    # the largest diagonal candidate of the ACGT columns so far, out of the frame

    def step(t, s):
        h_in = [0 | lead_border[0]] + [HOl[l][K - 1] for l in range(G - 1)]
        f_in = [0] + f_last[:-1]
        for l in range(G):
            j = t - l + lead
            diag0, up0[l] = up0[l], h_in[l]
            left = list(Hl[l])
            f, ho = f_in[l], up0[l]
            ds = []
            for q in range(K):
                floor = fl[l][(q + s) % K]
                assert floor == _add16(B, x * u_of(l, q, t))
                d = _add16(diag0 if q == 0 else left[q - 1], score(l, q, j))
                e = _hmax(El[l][q], HOl[l][q], floor)
                f = frame._hmax_shifted(f, ho) if f == 0 else _hmax(f, ho)
                h = _hmax(d, e, f)
                ho = _add16(h, -ox)
                Hl[l][q], El[l][q], HOl[l][q] = h, e, ho
                ds.append(d)
                if j < 0:                                            # left of the matrix: exactly the floor, the floor operand won
                    assert d <= floor and h == floor and e == floor, (l, q, t, j)
                elif j >= end:                                       # right of the last ACGT column: nothing new is offered
                    assert _i16(_add16(d, -floor)) <= offered[0], (l, q, t, j)
                else:
                    offered[0] = max(offered[0], _i16(_add16(d, -floor)))
            f_last[l] = f
            a = acc[l]
            for q in range(0, K, 2):
                slot = (q + s) % K
                a[slot] = _hmax(a[slot], ds[q], dprev[l][q + 1])
            for q in range(1, K, 2):
                dprev[l][q] = ds[q]
            a[s] = _add16(a[s], K * x)
            fl[l][s] = _add16(fl[l][s], K * x)
        lead_border[0] = _add16(lead_border[0], x)

    t = 0
    for s in range(s0, K):
        step(t, s)
        t += 1
    while t < steps:
        for s in range(K):
            step(t, s)
            t += 1
    assert t == steps
    best = 0
    for l in range(G):
        for q in range(0, K, 2):
            acc[l][q] = _hmax(acc[l][q], dprev[l][q + 1])
        for slot in range(K):
            best = max(best, _i16(_add16(acc[l][slot], -fl[l][slot])))
    return best


def _check(read, ref, scoring, G, K, cols=None):
    """The form the kernel would run on this pair (alone in its wave), and the repairing form whatever the pair."""
    exp = _oracle(read, ref, *scoring)
    form = REPAIR if needs_repair(ref) else TABLES
    got = sweep_score(read, ref, *scoring, G, K, form, cols)
    assert got == exp, (G, K, scoring, form, bytes(read), bytes(ref), got, exp)
    if form == TABLES:                                                # a clean pair in a wave that repairs
        assert sweep_score(read, ref, *scoring, G, K, REPAIR, cols) == exp
    return exp, form


SCORINGS = [sub + gaps for gaps in GAPS for sub in SUBS if rule_ok(*(sub + gaps))]


def test_the_scorings_cover_the_rule():
    assert (2, -1, -5, -1) in SCORINGS and (2, -1, -2, -3) not in SCORINGS and (5, -4, -5, -1) not in SCORINGS
    assert len(SCORINGS) >= 5


@pytest.mark.parametrize("scoring", SCORINGS, ids=lambda s: "%d_%d_%d_%d" % s)
def test_row_table_sweep_is_the_oracle(scoring):
    rng = np.random.default_rng(4000 + SCORINGS.index(scoring))
    forms = set()
    for case in range(120):
        G, K = frame.GEOMETRIES[int(rng.integers(0, len(frame.GEOMETRIES)))]
        read, ref = _related(rng, int(rng.integers(1, G * K + 1)), int(rng.integers(1, 15)))
        if case % 3 == 0:
            ref[int(rng.integers(0, len(ref))):] = 0                 # a NUL-padded short reference
        if case % 5 == 0:
            ref[0] = ord("N")                                        # column 0
        if case % 7 == 0 and last_acgt_end(ref) >= 2:
            ref[last_acgt_end(ref) - 2] = ord("x")                   # the column before the last ACGT base
        cols = last_acgt_end(ref) + int(rng.integers(0, 9)) if case % 2 else None
        forms.add(_check(read, ref, scoring, G, K, cols)[1])
    assert forms == {TABLES, REPAIR}


def test_the_plain_form_is_wrong_before_the_last_acgt_base():
    """... which is why such a wave repairs: the N scores 0 where the frame needs 2x, and the diagonal through it comes out short."""
    read = np.frombuffer(b"ACGTAACGT", dtype=np.uint8)
    ref = np.frombuffer(b"ACGTNACGT", dtype=np.uint8)
    scoring = (2, -1, -5, -1)
    exp = _oracle(read, ref, *scoring)
    assert exp == 16 and needs_repair(ref)
    for G, K in ((4, 4), (3, 4), (2, 6)):
        assert sweep_score(read, ref, *scoring, G, K, REPAIR) == exp
        assert sweep_score(read, ref, *scoring, G, K, TABLES) == exp - 2
    # after the last ACGT base the same N costs nothing
    tail = np.frombuffer(b"ACGTAACGTNN\0\0", dtype=np.uint8)
    assert not needs_repair(tail) and sweep_score(read, tail, *scoring, 4, 4, TABLES, cols=13) == _oracle(read, tail, *scoring) == 18


SHAPES = [(R, F, 16, 10) for R in (150, 160, 149, 159) for F in (1, 15, 16, 17)] + [(R, 9, 8, 12) for R in (83, 84, 95, 96)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-on-%dx%d" % s)
def test_kernel_shapes(shape):
    R, F, G, K = shape
    rng = np.random.default_rng(R * 1000 + F)
    read, ref = _related(rng, R, F)
    _check(read, ref, (2, -1, -5, -1), G, K, cols=F + 3)
    read = np.frombuffer(b"NnXN" * R, dtype=np.uint8)[:R]            # rows that score nothing: four equal bytes
    assert _check(read, ref, (2, -1, -5, -1), G, K)[0] == 0


def test_one_matching_base_at_every_cell():
    for G, K, R in ((4, 4, 16), (4, 4, 11), (3, 2, 6)):
        for F in (5, 6):
            for i in range(R):
                for j in range(F):
                    read, ref = np.full(R, ord("A"), dtype=np.uint8), np.full(F, ord("C"), dtype=np.uint8)
                    read[i], ref[j] = ord("G"), ord("G")
                    assert sweep_score(read, ref, 2, -1, -5, -1, G, K, TABLES, cols=F + (i + j) % 3) == 2, (G, K, R, F, i, j)


def test_the_window_at_the_rules_edges(monkeypatch):
    """The diagonal candidates of the columns that score 0 are never below B + x in rows 1 .. K-1 and B - (o - x) in a lane's
    row 0, and nothing else is; at the byte edges (largest byte 255, mismatch' = 0) and at the tilted window's
    upper edge the largest stays where sym_affine_tilt_ok puts it."""
    seen = []
    real = frame._hmax

    def spy(*patterns):
        seen.extend(patterns)
        return real(*patterns)

    monkeypatch.setattr(sys.modules[__name__], "_hmax", spy)
    seq = np.frombuffer(b"ACGTTGCAGTCATGCCATAGGTCAATCGGATTACAGCTTGAC", dtype=np.uint8)
    for (gap_open, gap_ext), (G, K, R, F) in (((-5, -1), (2, 4, 8, 8)), ((-7, -3), (3, 4, 11, 11)), ((-5, -2), (2, 4, 8, 30)),
                                              ((-4, 0), (2, 4, 5, 30)), ((-1, -1), (2, 6, 12, 20))):
        o, x = -gap_open, -gap_ext
        top = tilt_top_index(R, F, G, K)
        by_window = (WINDOW[1] - 1 - tilt_bias(1, -2 * x, gap_open, gap_ext) - x * top) // min(R, F)
        match = min(255 - o - x, by_window)                          # the largest byte is 255, or the window's edge comes first
        scoring = (match, -2 * x, gap_open, gap_ext)                 # mismatch' = 0
        assert rule_ok(*scoring) and not rule_ok(match, -2 * x - 1, gap_open, gap_ext)
        assert match == by_window or not rule_ok(match + 1, -2 * x, gap_open, gap_ext)
        B = tilt_bias(*scoring)
        read, ref = seq[:R], seq[:F]
        del seen[:]
        assert sweep_score(read, ref, *scoring, G, K, TABLES, cols=F) == _oracle(read, ref, *scoring) == min(R, F) * match
        assert min(seen) >= min(B + x, B - (o - x)) >= WINDOW[0]
        assert max(seen) <= B + x * top + min(R, F) * match <= WINDOW[1]
