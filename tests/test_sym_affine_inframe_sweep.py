"""The tilted biased int16 Smith-Waterman sweep with symmetric affine gaps AS score_kernel RUNS IT, restated on the CPU (no
GPU, no HIP code involved).  tests/test_sym_affine_tilted_sweep.py restates the frame -- cell (p, j) kept as value + B + x u,
u = p + j + c0, x = -extend, maxima on the bit patterns read as half floats -- and this file keeps its cell

    d = diag + S';  e = max3(E, HO, floor);  f = max(f, ho);  h = max3(d, e, f);  ho = h - (o - x)

and changes what surrounds it:

  * THE RUNNING MAXIMUM STAYS IN THE FRAME.  One accumulator per live anti-diagonal c = q + t of a lane, in the floors' slots.
    Rows go in pairs: the d of an even row q and the previous step's d of row q + 1 lie on the same c and enter its accumulator
    in one max3.  When row 0 completes its anti-diagonal the slot is recycled to c + K and the accumulator is carried over as
    acc + K x -- the same value read in the new frame, the addend the floor gets -- and keeps collecting.  The K accumulators
    take in the odd rows of the last step, leave the frame (acc - floor, plain int16) and are reduced once, after the last step.
  * THE HAND-OVER CARRIES ho.  A lane reads the `ho` of the last row of the lane above, not its h: that is F's source of its
    row 0 as it comes, and the diagonal of row 0 one step later, short of o - x -- which every profile score of a lane's row
    q == 0 carries (S' = S + 2x + (o - x) there, the zero slab included).  The moving border of the group's first lane is
    floor - (o - x) likewise.
  * THE REMAINDER RUNS THROUGH THE ROTATION.  steps % K steps run first as the LAST steps of a trip of K: the slots start out
    named as that step finds them and nothing is ever copied.

Every operand of every maximum is asserted to lie in [0x0400, 0x7BFF], carried accumulators included (F above the group's
first lane is the shift's zero, as in the other file), at small shapes and at the edge of cell_rules.h: sym_affine_tilt_ok,
B + x (rows + F - lead) + min(R, F) max(match, mismatch, 0) + 1 <= 0x7BFF.  A carried accumulator holds the largest cell the
lane has seen plus B + x u of a cell of the sweep, so the same rule bounds it.  Scores are compared exactly with
oracle.cpu_ref.score."""
import sys

import numpy as np
import pytest

import test_sym_affine_tilted_sweep as frame
from test_sym_affine_tilted_sweep import GAPS, SUBS, WINDOW, _add16, _i16, _oracle, _related, _remainder, _sub, tilt_bias, tilt_top_index


def _hmax(*patterns):
    return frame._hmax(*patterns)


def sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K):
    R, F = len(read), len(ref)
    rows = G * K
    assert R <= rows and K % 2 == 0
    o, x = -gap_open, -gap_ext
    ox = o - x                                                      # what an opening costs in the frame (may be negative)
    B = tilt_bias(match, mismatch, gap_open, gap_ext)
    S = [[0] * F for _ in range(rows)]                              # rows padded at the top score nothing
    for r in range(R):
        for j in range(F):
            S[rows - R + r][j] = _sub(read[r], ref[j], match, mismatch)
    lead = (rows - R) // K if rows > R else 0
    steps = F + G - 1 - lead

    def u_of(l, q, t):
        return l * (K - 1) + q + t + 2

    def profile(l, q, j):
        """S' of row q of lane l at column j; outside the columns: the zero slab"""
        return (S[l * K + q][j] if 0 <= j < F else 0) + 2 * x + (ox if q == 0 else 0)

    # every register by formula, as if step -1 had just run on cells that are all zero
    Hl = [[_add16(B, x * u_of(l, q, -1)) for q in range(K)] for l in range(G)]
    El = [list(row) for row in Hl]
    HOl = [[_add16(v, -ox) for v in row] for row in Hl]
    up0 = [_add16(B, x * u_of(l, -1, -1) - ox) for l in range(G)]   # ho of row -1 at step -1: row 0's diagonal at step 0
    f_last = [HOl[l][K - 1] for l in range(G)]
    s0 = K - steps % K                                              # the first step is step s0 of a trip (K: no remainder)
    fl = [[_add16(B, x * u_of(l, (i - s0) % K, 0)) for i in range(K)] for l in range(G)]     # slot i: c = (i - s0) % K, + K, ...
    acc = [list(row) for row in fl]                                 # an accumulator at its floor holds "0"
    dprev = [[_add16(B, x * u_of(l, q - 1, 0)) if q & 1 else None for q in range(K)] for l in range(G)]
    lead_border = [_add16(B, x * u_of(0, -1, 0) - ox)]              # ho of row -1 as the group's first lane reads it

    def step(t, s):
        """s: which slot holds the floor / accumulator of row 0 (row q: slot (q + s) % K)"""
        h_in = [0 | lead_border[0]] + [HOl[l][K - 1] for l in range(G - 1)]     # the shift's zero, the border OR-ed onto it
        f_in = [0] + f_last[:-1]
        for l in range(G):
            j = t - l + lead                                          # lanes outside [0, F) read the zero slab, unmasked
            diag0, up0[l] = up0[l], h_in[l]
            left = list(Hl[l])
            f, ho = f_in[l], up0[l]
            ds = []
            for q in range(K):
                floor = fl[l][(q + s) % K]
                assert floor == _add16(B, x * u_of(l, q, t))
                d = _add16(diag0 if q == 0 else left[q - 1], profile(l, q, j))
                e = _hmax(El[l][q], HOl[l][q], floor)
                f = frame._hmax_shifted(f, ho) if f == 0 else _hmax(f, ho)
                h = _hmax(d, e, f)
                ho = _add16(h, -ox)
                Hl[l][q], El[l][q], HOl[l][q] = h, e, ho
                ds.append(d)
            f_last[l] = f
            a = acc[l]
            for q in range(0, K, 2):
                slot = (q + s) % K
                a[slot] = _hmax(a[slot], ds[q], dprev[l][q + 1])
            for q in range(1, K, 2):
                dprev[l][q] = ds[q]
            # row 0's anti-diagonal is complete: the slot moves on to c + K, floor and accumulator alike
            a[s] = _add16(a[s], K * x)
            fl[l][s] = _add16(fl[l][s], K * x)
        lead_border[0] = _add16(lead_border[0], x)

    t = 0
    for s in range(s0, K):                                            # the remainder: the tail of a trip
        step(t, s)
        t += 1
    while t < steps:                                                  # trips of K steps: the slots change names
        for s in range(K):
            step(t, s)
            t += 1
    assert t == steps
    best = 0
    for l in range(G):                                                # the odd rows of the last step, then out of the frame
        for q in range(0, K, 2):
            acc[l][q] = _hmax(acc[l][q], dprev[l][q + 1])
        for slot in range(K):
            best = max(best, _i16(_add16(acc[l][slot], -fl[l][slot])))
    return best


def _check(read, ref, scoring, G, K):
    match, mismatch, gap_open, gap_ext = scoring
    exp = _oracle(read, ref, match, mismatch, gap_open, gap_ext)
    got = sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K)
    assert got == exp, (G, K, scoring, bytes(read), bytes(ref), got, exp)
    return exp


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("gaps", GAPS)
def test_inframe_sweep_is_the_oracle(gaps, sub):
    rng = np.random.default_rng(3000 * GAPS.index(gaps) + SUBS.index(sub))
    remainders = set()
    for case in range(150):
        G, K = frame.GEOMETRIES[int(rng.integers(0, len(frame.GEOMETRIES)))]
        read, ref = _related(rng, int(rng.integers(1, G * K + 1)), int(rng.integers(1, 15)))
        _check(read, ref, sub + gaps, G, K)
        r = _remainder(len(read), len(ref), G, K)
        remainders.add("0" if r == 0 else "1" if r == 1 else "K-1" if r == K - 1 else "mid")
    assert {"0", "1", "K-1"} <= remainders


SHAPES = [(R, F, 16, 10) for R in (150, 160, 141) for F in (1, 9, 10, 11, 37)] + [(96, 25, 8, 12)]
# ... and widths that leave 0, 1 and K - 1 remainder steps on the same geometries
SHAPES += [(150, 6, 16, 10), (150, 7, 16, 10), (150, 5, 16, 10), (96, 5, 8, 12), (96, 6, 8, 12), (96, 4, 8, 12)]


def test_the_shapes_cover_the_leads_and_remainders():
    leads = {(16 * 10 - R) // 10 for R, F, G, K in SHAPES if (G, K) == (16, 10)}
    assert leads == {0, 1}
    for G, K in ((16, 10), (8, 12)):
        rem = {_remainder(R, F, G, K) for R, F, g, k in SHAPES if (g, k) == (G, K)}
        assert {0, 1, K - 1} <= rem, (G, K, rem)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-on-%dx%d" % s)
def test_kernel_shapes(shape):
    R, F, G, K = shape
    rng = np.random.default_rng(R * 1000 + F)
    for scoring in ((2, -1, -5, -1), (5, -4, -2, -3)):
        _check(*_related(rng, R, F), scoring, G, K)
    # a read of bases that score nothing: every cell stays at its floor, the score is 0
    read = np.frombuffer(b"NnXN" * R, dtype=np.uint8)[:R]
    assert _check(read, _related(rng, R, F)[1], (2, -1, -5, -1), G, K) == 0


@pytest.mark.parametrize("geo", ((4, 4), (2, 6), (3, 2)), ids=lambda g: "%dx%d" % g)
def test_every_remainder(geo):
    G, K = geo
    rng = np.random.default_rng(177 + G * K)
    seen = set()
    for R in (G * K, G * K - K - 1 if G > 1 else 1):
        for F in range(1, 2 * K + 2):
            read, ref = _related(rng, R, F)
            for gaps, sub in zip(GAPS, SUBS + SUBS):
                _check(read, ref, sub + gaps, G, K)
            seen.add(_remainder(R, F, G, K))
    assert seen == set(range(K))


def test_one_matching_base_at_every_cell():
    """All mismatches but one matching base at (i, j): only that cell can supply the score -- the first anti-diagonal (0, 0),
    the last (R - 1, F - 1), a lane's first and last row, the odd rows of the last step."""
    match, mismatch = 2, -1
    for G, K, R in ((4, 4, 16), (4, 4, 13), (4, 4, 5), (3, 2, 6)):
        for F in (5, 6):
            for gap_open, gap_ext in GAPS:
                for i in range(R):
                    for j in range(F):
                        read, ref = np.full(R, ord("A"), dtype=np.uint8), np.full(F, ord("C"), dtype=np.uint8)
                        read[i], ref[j] = ord("G"), ord("G")
                        assert sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K) == match, (G, K, R, F, i, j)


@pytest.mark.parametrize("shape", ((150, 11, 16, 10), (160, 9, 16, 10), (96, 25, 8, 12)), ids=lambda s: "%dx%d-on-%dx%d" % s)
def test_the_first_and_the_last_anti_diagonal(shape):
    R, F, G, K = shape
    for i, j in ((0, 0), (R - 1, F - 1)):
        read, ref = np.full(R, ord("A"), dtype=np.uint8), np.full(F, ord("C"), dtype=np.uint8)
        read[i], ref[j] = ord("G"), ord("G")
        assert _check(read, ref, (2, -1, -5, -1), G, K) == 2


def test_a_diagonal_across_the_lane_boundary():
    """Two matching bases in a row, the second in a lane's row q == 0: its score arrives by the diagonal from the lane above,
    through the handed-over ho and the o - x of the profile -- for every opening cost in the frame, negative ones included."""
    for G, K, R, F in ((4, 4, 16, 7), (4, 4, 14, 7), (3, 2, 6, 5), (16, 10, 150, 9)):
        rows = G * K
        hits = 0
        for i in range(1, R):
            if (rows - R + i) % K:
                continue
            for j in ((1, F - 1) if K == 10 else range(1, F)):
                for scoring in ((2, -1, -5, -1), (3, 1, -2, -3), (5, -4, -4, 0)):
                    read, ref = np.full(R, ord("A"), dtype=np.uint8), np.full(F, ord("C"), dtype=np.uint8)
                    read[i - 1], ref[j - 1], read[i], ref[j] = ord("G"), ord("G"), ord("T"), ord("T")
                    assert _check(read, ref, scoring, G, K) >= 2 * scoring[0]
                    hits += 1
        assert hits


def _rule_edge_match(R, F, G, K, mismatch, gap_open, gap_ext):
    """The largest match score cell_rules.h: sym_affine_tilt_ok lets run tilted on this shape."""
    B = tilt_bias(1, mismatch, gap_open, gap_ext)
    return (WINDOW[1] - 1 - B - (-gap_ext) * tilt_top_index(R, F, G, K)) // min(R, F)


def test_the_rules_edge(monkeypatch):
    """At the last match score the rule admits every operand stays inside the window, carried accumulators included, and the
    accumulators do climb with the tilt: a read that matches the first bases of a longer reference reaches the full score
    early in the last lane, and the accumulator of that anti-diagonal's slot carries it -- the score plus B + x u of the
    slot's current frame -- to the end of the sweep."""
    seen = []
    real = frame._hmax

    def spy(*patterns):
        seen.extend(patterns)
        return real(*patterns)

    monkeypatch.setattr(sys.modules[__name__], "_hmax", spy)
    seq = np.frombuffer(b"ACGTTGCAGTCATGCCATAGGTCAATCGGATTACAGCTTGAC", dtype=np.uint8)
    for (gap_open, gap_ext), (G, K, R, F) in (((-5, -1), (2, 4, 8, 8)), ((-5, -1), (4, 2, 8, 8)), ((-7, -3), (3, 4, 11, 11)),
                                              ((-5, -2), (2, 4, 8, 30)), ((-4, 0), (2, 4, 5, 30)), ((-2, -3), (2, 6, 12, 41))):
        read, ref = seq[:R], seq[:F]
        match = _rule_edge_match(R, F, G, K, -1, gap_open, gap_ext)
        B, x, top = tilt_bias(match, -1, gap_open, gap_ext), -gap_ext, tilt_top_index(R, F, G, K)
        assert B + x * top + R * match + 1 <= WINDOW[1] < B + x * top + R * (match + 1) + 1
        del seen[:]
        assert _check(read, ref, (match, -1, gap_open, gap_ext), G, K) == R * match
        assert WINDOW[0] <= min(seen) and max(seen) <= B + x * top + R * match
        if F > R:
            # carried from column R - 1 into the last two trips (a slot is an operand on every second step, in the frame
            # it has then), far beyond the cell itself at u = rows + R
            assert G * K + R < top - 2 * K and max(seen) >= B + x * (top - 2 * K) + R * match
