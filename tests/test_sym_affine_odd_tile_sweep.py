"""The row-table step of the tilted int16 Smith-Waterman sweep with symmetric affine gaps on a tile with an ODD number of rows
per lane, as score_kernel<8, 19, kAlgSW, kGapAffineSym> runs it (dp_kernels.hip.h: TABLES_ONLY), restated on the CPU (no GPU, no
HIP code involved).  It is the restatement of tests/test_sym_affine_row_tables_sweep.py -- the same cell, hand-over, floors, row
tables, plain and repairing form -- with what an odd K changes:

  * rows 0 .. K - 2 enter the accumulators in pairs (an even row q with the previous step's row q + 1: the same anti-diagonal);
    the last row, q = K - 1, is even, has no partner and enters the slot of its own anti-diagonal alone, at once, through a
    two-operand maximum.  Asserted here: every diagonal candidate of the sweep enters exactly ONE slot, before that slot moves
    on, and the score that leaves the frame is the largest candidate there was;
  * after the last step only the odd rows' candidates wait to be entered;
  * the selector stream is the compact one: 16 bits per column, {ca, 4 + cb}, widened to {ca, 0x0c, 4 + cb, 0x0c} by one byte
    permute against 0x0c0c0c0c -- restated with the permute's own selector constant, both pairs of a register.

Scores are compared exactly with oracle.cpu_ref.score; the even-K models of the older file run through this restatement too.
At the last match score the rule admits on 8 x 19 (side_tile_edge_match) the operands of every maximum are collected and bounded:
the constructions of tests/test_gpu_sym_affine_side_tile_edges.py (edge_quarters), whose operands the GPU cannot show."""
import numpy as np
import pytest

import test_sym_affine_tilted_sweep as frame
from test_sym_affine_row_tables_sweep import REPAIR, TABLES, last_acgt_end, needs_repair, rule_ok
from test_sym_affine_row_tables_sweep import sweep_score as even_sweep_score
from test_sym_affine_tilted_sweep import _CLASS, _add16, _i16, _oracle, _related, tilt_bias

SEL_ZERO4, SEL_WIDEN = 0x0C0C0C0C, 0x04010400           # dp_kernels.hip.h: kSelZero4, kSelWiden
ODD_GEOMETRIES = ((1, 3), (2, 3), (4, 3), (3, 5), (2, 7), (1, 1), (3, 1))
SCORING = (2, -1, -5, -1)


def _perm(hi, lo, sel):
    """v_perm_b32: byte i of the result is byte sel[i] of {hi, lo} (0 .. 3 lo, 4 .. 7 hi), 0x00 for selector 0x0c"""
    src = [(lo >> (8 * i)) & 0xFF for i in range(4)] + [(hi >> (8 * i)) & 0xFF for i in range(4)]
    out = 0
    for i in range(4):
        b = (sel >> (8 * i)) & 0xFF
        assert b <= 7 or b == 0x0C, hex(sel)
        out |= (0 if b == 0x0C else src[b]) << (8 * i)
    return out


def compact_entry(base_a, base_b):
    """One column of a group's stream: {ca, 4 + cb}, 0x0c where the base is no ACGT (None: a pad column)"""
    ca = _CLASS.get(int(base_a), 0) if base_a is not None else 0
    cb = _CLASS.get(int(base_b), 0) if base_b is not None else 0
    return (ca - 1 if 1 <= ca <= 4 else 0x0C) | (cb + 3 if 1 <= cb <= 4 else 0x0C) << 8


def test_the_widening_permute():
    for a in (None,) + tuple(b"ACGTNx\0"):
        for b in (None,) + tuple(b"ACGTNx\0"):
            entry = compact_entry(a, b)
            assert 0 <= entry <= 0xFFFF
            sel = _perm(SEL_ZERO4, entry, SEL_WIDEN)
            assert sel == (entry & 0xFF) | 0x0C << 8 | (entry >> 8) << 16 | 0x0C << 24
            Ta, Tb = 0x44332211, 0x88776655                         # the four bytes of a row, pair A and pair B
            s = _perm(Tb, Ta, sel)
            ca, cb = entry & 0xFF, entry >> 8
            assert s & 0xFFFF == (0 if ca == 0x0C else 0x11 * (ca + 1)) and s >> 16 == (0 if cb == 0x0C else 0x11 * (cb + 1))
            # the repairing form reads bit 3 of the two selector bytes
            assert ((sel >> 3) & 0x00010001) == (1 if ca == 0x0C else 0) | (1 if cb == 0x0C else 0) << 16


def sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K, form, cols=None):
    R = len(read)
    rows = G * K
    assert R <= rows and rule_ok(match, mismatch, gap_open, gap_ext)
    o, x = -gap_open, -gap_ext
    ox = o - x
    B = tilt_bias(match, mismatch, gap_open, gap_ext)
    end = last_acgt_end(ref)
    F = end if cols is None else cols
    assert F >= end
    T = []
    for p in range(rows):
        a = _CLASS.get(int(read[p - (rows - R)]), 0) if p >= rows - R else 0
        row = [(match if a == c else mismatch) + 2 * x if 1 <= a <= 4 else 2 * x for c in (1, 2, 3, 4)]
        row = [v + (ox if p % K == 0 else 0) for v in row]
        assert all(0 <= v <= 255 for v in row), row
        T.append(sum(v << (8 * i) for i, v in enumerate(row)))
    pad = G + 4                                                      # row_table_pad
    stream = {j: compact_entry(ref[j] if 0 <= j < len(ref) else None, None) for j in range(-pad, F + pad)}
    lead = (rows - R) // K if rows > R else 0
    steps = F + G - 1 - lead

    def u_of(l, q, t):
        return l * (K - 1) + q + t + 2

    def score(l, q, j):
        assert -(G - 1) <= j <= F + G - 2, j                         # what the sweep reads of the pads (the prefetch: two more)
        s = _perm(0, T[l * K + q], _perm(SEL_ZERO4, stream[j], SEL_WIDEN)) & 0xFFFF
        if form == REPAIR and stream[j] & 0xFF == 0x0C:
            s |= 2 * x + (ox if q == 0 else 0)
        return s

    Hl = [[_add16(B, x * u_of(l, q, -1)) for q in range(K)] for l in range(G)]
    El = [list(row) for row in Hl]
    HOl = [[_add16(v, -ox) for v in row] for row in Hl]
    up0 = [_add16(B, x * u_of(l, -1, -1) - ox) for l in range(G)]
    f_last = [HOl[l][K - 1] for l in range(G)]
    s0 = K - steps % K
    fl = [[_add16(B, x * u_of(l, (i - s0) % K, 0)) for i in range(K)] for l in range(G)]
    acc = [list(row) for row in fl]
    slot_c = [[(i - s0) % K for i in range(K)] for _ in range(G)]    # the anti-diagonal c = q + t a slot stands for
    dprev = [[_add16(B, x * u_of(l, q - 1, 0)) if q & 1 else None for q in range(K)] for l in range(G)]
    dprev_c = [[None] * K for _ in range(G)]                         # ... and the one a waiting candidate lies on
    lead_border = [_add16(B, x * u_of(0, -1, 0) - ox)]
    seen = {"offered": 0, "entered": 0, "computed": 0}

    def enter(l, slot, d, c):
        assert slot_c[l][slot] == c, (l, slot, c, slot_c[l][slot])    # the slot still stands for the candidate's anti-diagonal
        seen["entered"] += 1

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
                e = frame._hmax(El[l][q], HOl[l][q], floor)
                f = frame._hmax_shifted(f, ho) if f == 0 else frame._hmax(f, ho)
                h = frame._hmax(d, e, f)
                ho = _add16(h, -ox)
                Hl[l][q], El[l][q], HOl[l][q] = h, e, ho
                ds.append(d)
                seen["computed"] += 1
                seen["offered"] = max(seen["offered"], _i16(_add16(d, -floor)))
            f_last[l] = f
            a = acc[l]
            for q in range(0, K, 2):
                slot = (q + s) % K
                enter(l, slot, ds[q], q + t)
                if q + 1 < K:
                    a[slot] = frame._hmax(a[slot], ds[q], dprev[l][q + 1])
                    if dprev_c[l][q + 1] is not None:
                        enter(l, slot, dprev[l][q + 1], dprev_c[l][q + 1])
                else:
                    a[slot] = frame._hmax(a[slot], ds[q])             # the unpaired last row of an odd K
            for q in range(1, K, 2):
                dprev[l][q], dprev_c[l][q] = ds[q], q + t
            assert slot_c[l][s] == t                                 # row 0 has completed anti-diagonal c = t: the slot moves on
            a[s] = _add16(a[s], K * x)
            fl[l][s] = _add16(fl[l][s], K * x)
            slot_c[l][s] += K
        lead_border[0] = _add16(lead_border[0], x)

    t = 0
    for s in range(s0 % K, K if s0 < K else 0):
        step(t, s)
        t += 1
    while t < steps:
        for s in range(K):
            step(t, s)
            t += 1
    assert t == steps
    best = 0
    for l in range(G):
        for q in range(0, K - 1, 2):
            if dprev_c[l][q + 1] is not None:
                enter(l, q, dprev[l][q + 1], dprev_c[l][q + 1])
            acc[l][q] = frame._hmax(acc[l][q], dprev[l][q + 1])
        for slot in range(K):
            best = max(best, _i16(_add16(acc[l][slot], -fl[l][slot])))
    assert seen["entered"] == seen["computed"]                       # every candidate entered a slot, once
    assert best == max(0, seen["offered"])                           # ... and the largest of them is what leaves the frame
    return best


def _check(read, ref, scoring, G, K, cols=None):
    exp = _oracle(read, ref, *scoring)
    form = REPAIR if needs_repair(ref) else TABLES
    got = sweep_score(read, ref, *scoring, G, K, form, cols)
    assert got == exp, (G, K, scoring, form, bytes(read), bytes(ref), got, exp)
    if form == TABLES:
        assert sweep_score(read, ref, *scoring, G, K, REPAIR, cols) == exp
    return exp, form


def test_even_tiles_agree_with_the_older_restatement():
    rng = np.random.default_rng(77)
    for _ in range(40):
        G, K = frame.GEOMETRIES[int(rng.integers(0, len(frame.GEOMETRIES)))]
        read, ref = _related(rng, int(rng.integers(1, G * K + 1)), int(rng.integers(1, 13)))
        form = REPAIR if needs_repair(ref) else TABLES
        cols = last_acgt_end(ref) + int(rng.integers(0, 5))
        assert sweep_score(read, ref, *SCORING, G, K, form, cols) == even_sweep_score(read, ref, *SCORING, G, K, form, cols)


@pytest.mark.parametrize("scoring", ((2, -1, -5, -1), (3, 1, -5, -1), (2, -1, -1, -1), (2, 0, 0, 0), (5, -2, -7, -1)), ids=lambda s: "%d_%d_%d_%d" % s)
def test_odd_tile_sweep_is_the_oracle(scoring):
    assert rule_ok(*scoring)
    rng = np.random.default_rng(9000 + sum(scoring))
    forms, remainders = set(), set()
    for case in range(150):
        G, K = ODD_GEOMETRIES[int(rng.integers(0, len(ODD_GEOMETRIES)))]
        read, ref = _related(rng, int(rng.integers(1, G * K + 1)), int(rng.integers(1, 15)))
        if case % 3 == 0:
            ref[int(rng.integers(0, len(ref))):] = 0
        if case % 5 == 0:
            ref[0] = ord("N")
        if case % 7 == 0 and last_acgt_end(ref) >= 2:
            ref[last_acgt_end(ref) - 2] = ord("x")
        cols = last_acgt_end(ref) + int(rng.integers(0, 9)) if case % 2 else None
        forms.add(_check(read, ref, scoring, G, K, cols)[1])
        remainders.add((K, frame._remainder(len(read), cols if cols is not None else last_acgt_end(ref), G, K)))
    assert forms == {TABLES, REPAIR}
    assert {(3, 0), (3, 1), (3, 2)} <= remainders and len({r for k, r in remainders if k == 5}) >= 3


KERNEL_SHAPES = [(R, F) for R in (132, 133, 150, 151, 152) for F in (1, 7, 19)] + [(150, 20), (152, 37), (151, 38), (129, 8), (1, 9), (1, 1)]


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_8x19_tile(shape):
    R, F = shape
    rng = np.random.default_rng(R * 1000 + F)
    read, ref = _related(rng, R, F)
    _check(read, ref, SCORING, 8, 19, cols=F + 2)
    read = np.frombuffer(b"NnXN" * R, dtype=np.uint8)[:R]
    assert _check(read, ref, SCORING, 8, 19)[0] == 0


def side_tile_edge_match(R, F, mismatch, gap_open, gap_ext, top_index=None):
    """The last match score cell_rules.h: sym_affine_tilt_ok lets the 8 x 19 tile run on R x F, restated:
    B + x * (rows + F - lead) + min(R, F) * match + 1 <= 0x7BFF.  top_index: another top index than the rule's."""
    B, x = tilt_bias(1, mismatch, gap_open, gap_ext), -gap_ext
    top = frame.tilt_top_index(R, F, 8, 19) if top_index is None else top_index
    match = (frame.WINDOW[1] - 1 - B - x * top) // min(R, F)
    assert match > 0 and tilt_bias(match, mismatch, gap_open, gap_ext) == B
    # ... inside the plain biased form's window (sym_affine_max3_ok) and the bytes of the row tables, one match score further too
    plain = 1024 - gap_open - gap_ext + max(0, -mismatch)
    assert plain - 1024 <= 1024 and plain + min(R, F) * (match + 1) + 1 <= frame.WINDOW[1]
    assert rule_ok(match + 1, mismatch, gap_open, gap_ext)
    return match


def edge_quarters(R, F, seed):
    """The four constructions that put the largest score a shape holds against the top of the tilted window: the read is the
    reference's LAST R bases (the full score lands in the last row at the last column, where the tilt is largest), its FIRST R
    bases (the maximum is found early and rides the accumulators to the top index), and each again with one N inside the
    matched piece of the reference (one base short, the repairing form).  -> [(name, read, ref, clean)]"""
    assert F >= R
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for name, at in (("last", F - R), ("first", 0)):
        ref = acgt[rng.integers(0, 4, size=F)].copy()
        read = ref[at:at + R].copy()
        out.append((name, read, ref, True))
        dirty = ref.copy()
        dirty[at + int(rng.integers(1, R - 1))] = ord("N")
        assert needs_repair(dirty)
        out.append((name + "-N", read, dirty, False))
    return out


EDGE_SCORINGS = ((-1, -5, -1), (-20, -24, -20))          # (mismatch, open, extend): score-dominated, tilt-dominated (x = 20: 380 per trip)
EDGE_MATCHES = {(152, 152, -1): 200, (152, 152, -20): 161, (133, 160, -1): 228, (133, 160, -20): 184}


@pytest.mark.parametrize("gaps", EDGE_SCORINGS, ids=lambda s: "%d_%d_%d" % s)
@pytest.mark.parametrize("shape", ((152, 152), (133, 160)), ids=lambda s: "%dx%d" % s)
def test_the_8x19_tile_at_the_windows_upper_edge(monkeypatch, shape, gaps):
    """The last match score the rule admits on the 8 x 19 tile: the sweep is the oracle and EVERY operand of every maximum, the
    accumulators included (acc[slot] += K x once per trip, up to the top index), lies in [0x0400, 0x7BFF] -- seen here, operand
    by operand, where a GPU test could only infer it from a wrong score.  The largest operand is the rule's own bound less its
    one spare unit where the full score lands in the last cell, and within two trips of it where it is carried there."""
    R, F = shape
    mismatch, gap_open, gap_ext = gaps
    match = side_tile_edge_match(R, F, mismatch, gap_open, gap_ext)
    assert match == EDGE_MATCHES[(R, F, mismatch)]
    scoring = (match, mismatch, gap_open, gap_ext)
    B, x, top = tilt_bias(*scoring), -gap_ext, frame.tilt_top_index(R, F, 8, 19)
    assert B + x * top + R * match + 1 <= frame.WINDOW[1] < B + x * top + R * (match + 1) + 1
    seen = []
    real = frame._hmax

    def spy(*patterns):
        seen.extend(patterns)
        return real(*patterns)

    monkeypatch.setattr(frame, "_hmax", spy)
    for name, read, ref, clean in edge_quarters(R, F, seed=R + F):
        del seen[:]
        exp = _oracle(read, ref, *scoring)
        got = sweep_score(read, ref, *scoring, 8, 19, TABLES if clean else REPAIR)
        assert got == exp and (exp == R * match if clean else (R - 1) * match <= exp < R * match), (name, got, exp)
        assert frame.WINDOW[0] <= min(seen) and max(seen) <= B + x * top + R * match, (name, hex(min(seen)), hex(max(seen)))
        if clean and name == "last":
            assert max(seen) == B + x * top + R * match, (name, max(seen))
        elif clean:
            assert max(seen) >= B + x * (top - 2 * 19) + R * match, (name, max(seen))


def test_one_matching_base_at_every_cell():
    """... of every row of an odd tile, the unpaired last row of every lane included, at both parities of the step count"""
    for G, K, R in ((3, 3, 9), (2, 5, 10), (2, 5, 7), (4, 3, 11)):
        for F in (5, 6):
            for i in range(R):
                for j in range(F):
                    read, ref = np.full(R, ord("A"), dtype=np.uint8), np.full(F, ord("C"), dtype=np.uint8)
                    read[i], ref[j] = ord("G"), ord("G")
                    assert sweep_score(read, ref, *SCORING, G, K, TABLES, cols=F + (i + j) % 3) == 2, (G, K, R, F, i, j)
