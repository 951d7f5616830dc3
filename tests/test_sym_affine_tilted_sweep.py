"""The TILTED biased form of the int16 Smith-Waterman sweep with symmetric affine gaps, restated on the CPU (no GPU, no HIP
code involved) the way tests/test_sym_affine_max3_sweep.py restates the plain biased form.  Cell (p, j) -- p the padded row, j
the column -- is kept as value + B + x * u with u = p + j + c0, x = -extend: in that frame an extension costs nothing,

    d = diag + S'            S' = S + 2x (the query profile carries the 2x, the zero slab too)
    e = max3(E, HO, floor)   floor = B + x * u, the zero of the cell's own frame
    f = max(f, ho)
    h = max3(d, e, f)
    ho = h - (o - x)         o = -open

with plain 16-bit adds that wrap and every maximum taken ON THE BIT PATTERNS READ AS HALF FLOATS, which is an integer maximum
while every operand lies in [0x0400, 0x7BFF]; this file asserts that of every operand of every maximum but one: F of the row
above the group's first lane is the zero the lane shift delivers there (+0.0, which loses to every pattern of the window).

The sweep runs as score_kernel runs it: lane groups of G lanes with K rows each, rows padded at the top, the sweep started
`lead` lanes down, unmasked steps on both sides of the reference.  Lane l at step t holds row q of its rows at
u = l (K - 1) + q + t + 2 (c0 = 2 - lead: the smallest u any register ever carries is 0), so the floor of a cell depends on
c = q + t alone within a lane: K floor registers, slot c % K, each used by one row per step and moved K x on when its
anti-diagonal c is complete.  The running maximum cannot mix tilts either: one accumulator per live c in the same slots, fed
with the step's diag + S' and the previous step's two at a time on every second step, taken out of the frame (acc - floor, plain
int16) when its c is complete, i.e. once per step.  steps % K remainder steps come first -- they feed every diag + S' singly
and rotate the slots by copying -- then trips of K steps in which the slots only change names.

B = 1024 + max(o - x, m, 0), m = the most a substitution score takes off a cell; the largest u a maximum sees is
rows + F - lead.  Scores are compared exactly with oracle.cpu_ref.score.  K is even here as in the kernel (Geo: static_assert),
which the two-step feeding relies on; the two odd-K models of the plain form's file are replaced by even ones."""
import sys

import numpy as np
import pytest

from oracle import cpu_ref

_CLASS = {ord(c): k for k, cs in ((1, "Aa"), (2, "Tt"), (3, "Cc"), (4, "Gg"), (5, "Nn")) for c in cs}      # DefaultKernel.h:43-60

GAPS = ((-5, -1), (-1, -1), (-2, -3), (-4, 0), (0, 0))          # (open, extend) of tests/test_gpu_sym_affine_sweep.py
SUBS = ((2, -1), (5, -4), (3, 1))                               # ... its substitution scores, and a positive mismatch score
GEOMETRIES = ((1, 2), (2, 2), (1, 4), (3, 2), (4, 4), (8, 2), (5, 4), (2, 6), (3, 4))      # (G, K) of the model, K even

WINDOW = (0x0400, 0x7BFF)
_HALF = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float64).tolist()


def _sub(a, b, match, mismatch):
    ca, cb = _CLASS.get(int(a), 0), _CLASS.get(int(b), 0)
    if 1 <= ca <= 4 and 1 <= cb <= 4:
        return match if ca == cb else mismatch
    return 0


def _add16(a, b):
    """v_pk_add_u16 / v_pk_sub_i16 without a clamp: 16 bits, wraps."""
    return (a + b) & 0xFFFF


def _i16(a):
    return a - 0x10000 if a & 0x8000 else a


def _hmax(*patterns):
    """A half-float maximum of bit patterns, every operand inside the window."""
    for p in patterns:
        assert WINDOW[0] <= p <= WINDOW[1], ("operand outside the window", hex(p))
    return max(patterns, key=_HALF.__getitem__)


def _hmax_shifted(f, ho):
    """max(f, ho) where f may be the zero a lane shift delivers in a group's first lane: +0.0"""
    if f == 0:
        assert WINDOW[0] <= ho <= WINDOW[1], ("operand outside the window", hex(ho))
        return max((f, ho), key=_HALF.__getitem__)
    return _hmax(f, ho)


def tilt_bias(match, mismatch, gap_open, gap_ext):
    return 1024 + max(-gap_open + gap_ext, -mismatch, -match, 0)


def tilt_top_index(R, F, G, K):
    """The largest u = p + j + c0 an operand of a maximum carries: the last lane's last row at the last step."""
    rows = G * K
    lead = (rows - R) // K if rows > R else 0
    return rows + F - lead


def sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K, extra_steps=0):
    """extra_steps: further unmasked steps past the sweep's end (they must not change the result)."""
    R, F = len(read), len(ref)
    rows = G * K
    assert R <= rows and K % 2 == 0
    o, x = -gap_open, -gap_ext
    B = tilt_bias(match, mismatch, gap_open, gap_ext)
    S = np.zeros((rows, F), dtype=np.int64)                         # rows padded at the top score nothing
    for r in range(R):
        for j in range(F):
            S[rows - R + r, j] = _sub(read[r], ref[j], match, mismatch)
    lead = (rows - R) // K if rows > R else 0
    ox = o - x                                                      # what an opening costs in the frame (may be negative)

    def u_of(l, q, t):
        return l * (K - 1) + q + t + 2

    # every register by formula, as if step -1 had just run on cells that are all zero
    Hl = [[_add16(B, x * u_of(l, q, -1)) for q in range(K)] for l in range(G)]
    El = [list(row) for row in Hl]
    HOl = [[_add16(v, -ox) for v in row] for row in Hl]
    up0 = [_add16(B, x * u_of(l, -1, -1)) for l in range(G)]
    h_last = [Hl[l][K - 1] for l in range(G)]
    f_last = [_add16(h_last[l], -ox) for l in range(G)]
    fl = [[_add16(B, x * u_of(l, q, 0)) for q in range(K)] for l in range(G)]       # slot q: the floor of c = q (+ K, 2K, ...)
    acc = [list(row) for row in fl]                                 # an accumulator at its floor holds "0"
    dprev = [[None] * K for _ in range(G)]
    best = [0] * G                                                  # plain int16, the score itself
    lead_border = [_add16(B, x * u_of(0, -1, 0))]                   # row -1 as the group's first lane sees it: one x more per step

    def step(t, s, kind):
        """s: which slot holds the floor / accumulator of row 0 (row q: slot (q + s) % K); kind: how the step feeds the
        accumulators -- 'all' every diag + S' singly, 'none' only row 0's (the others wait in dprev), 'pair' with dprev."""
        h_in = [0 | lead_border[0]] + h_last[:-1]                     # the shift's zero, the border OR-ed onto it
        f_in = [0] + f_last[:-1]
        for l in range(G):
            j = t - l + lead                                          # lanes outside [0, F) read the zero slab, unmasked
            sc = S[l * K:(l + 1) * K, j] if 0 <= j < F else np.zeros(K, dtype=np.int64)
            diag0, up0[l] = up0[l], h_in[l]
            left = list(Hl[l])
            f, ho = f_in[l], _add16(up0[l], -ox)
            ds = []
            for q in range(K):
                floor = fl[l][(q + s) % K]
                assert floor == _add16(B, x * u_of(l, q, t))
                d = _add16(diag0 if q == 0 else left[q - 1], int(sc[q]) + 2 * x)
                e = _hmax(El[l][q], HOl[l][q], floor)
                f = _hmax_shifted(f, ho)
                h = _hmax(d, e, f)
                ho = _add16(h, -ox)
                Hl[l][q], El[l][q], HOl[l][q] = h, e, ho
                ds.append(d)
            h_last[l], f_last[l] = h, f
            a = acc[l]
            if kind == "all":
                for q in range(K):
                    a[(q + s) % K] = _hmax(a[(q + s) % K], ds[q])
            elif kind == "none":
                a[s % K] = _hmax(a[s % K], ds[0])
            else:
                for q in range(K):
                    slot = (q + s) % K
                    if q == K - 1:
                        a[slot] = ds[q]                               # a new anti-diagonal: its first cell
                    elif q == K - 2:
                        a[slot] = _hmax(ds[q], dprev[l][q + 1])       # ... its first two
                    else:
                        a[slot] = _hmax(a[slot], ds[q], dprev[l][q + 1])
            dprev[l] = ds
            # row 0's anti-diagonal is complete: out of the frame, and the slot's floor moves on to c + K
            s0 = s % K
            best[l] = max(best[l], _i16(_add16(a[s0], -fl[l][s0])))
            fl[l][s0] = _add16(fl[l][s0], K * x)
        lead_border[0] = _add16(lead_border[0], x)

    steps = F + G - 1 - lead + extra_steps
    t = 0
    for _ in range(steps % K):                                        # remainder steps first: slots rotate by copying
        step(t, 0, "all")
        for l in range(G):
            fl[l] = fl[l][1:] + fl[l][:1]
            acc[l] = acc[l][1:] + [fl[l][K - 1]]
        t += 1
    while t < steps:                                                  # trips of K steps: the slots change names
        for s in range(K):
            step(t, s, "pair" if s & 1 else "none")
            t += 1
    for l in range(G):                                                # the anti-diagonals still open
        for slot in range(K):
            best[l] = max(best[l], _i16(_add16(acc[l][slot], -fl[l][slot])))
    return max(best)


def _oracle(read, ref, match, mismatch, gap_open, gap_ext):
    sc = cpu_ref.Scoring.make(match, mismatch, -3, -3, gap_open, gap_ext, gap_open, gap_ext)
    return int(cpu_ref.score(0, read[None, :], ref[None, :], sc, affine=True)[0])


def _related(rng, R, F):
    alphabet = np.frombuffer(b"ACGTACGTACGTACGTNn", dtype=np.uint8)                # mostly ACGT, some bases that score nothing
    ref = alphabet[rng.integers(0, len(alphabet), size=F)].copy()
    read = alphabet[rng.integers(0, len(alphabet), size=R)].copy()
    if rng.random() < 0.7:                                          # a piece of the reference, so that alignments are long
        m = int(rng.integers(1, min(R, F) + 1))
        a, b = int(rng.integers(0, F - m + 1)), int(rng.integers(0, R - m + 1))
        read[b:b + m] = ref[a:a + m]
        if m > 3 and rng.random() < 0.6:                            # ... with a gap in it
            cut = int(rng.integers(1, m - 1))
            read[b + cut:b + m - 1] = read[b + cut + 1:b + m].copy()
    return read, ref


def _remainder(R, F, G, K):
    rows = G * K
    lead = (rows - R) // K if rows > R else 0
    return (F + G - 1 - lead) % K


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("gaps", GAPS)
def test_tilted_sweep_is_the_oracle(gaps, sub):
    rng = np.random.default_rng(2000 * GAPS.index(gaps) + SUBS.index(sub))
    (gap_open, gap_ext), (match, mismatch) = gaps, sub
    remainders = set()
    for case in range(200):
        G, K = GEOMETRIES[int(rng.integers(0, len(GEOMETRIES)))]
        read, ref = _related(rng, int(rng.integers(1, G * K + 1)), int(rng.integers(1, 15)))
        exp = _oracle(read, ref, match, mismatch, gap_open, gap_ext)
        got = sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K)
        assert got == exp, (case, G, K, bytes(read), bytes(ref), got, exp)
        r = _remainder(len(read), len(ref), G, K)
        remainders.add("0" if r == 0 else "1" if r == 1 else "K-1" if r == K - 1 else "mid")
    assert {"0", "1", "K-1"} <= remainders


@pytest.mark.parametrize("shape", ((1, 1, 1, 2), (10, 7, 2, 6), (10, 7, 4, 4), (33, 64, 4, 10), (33, 64, 6, 6)),
                         ids=lambda s: "%dx%d-on-%dx%d" % s)
def test_fixed_shapes(shape):
    R, F, G, K = shape
    rng = np.random.default_rng(R * 1000 + F)
    pairs = [_related(rng, R, F) for _ in range(3)]
    for gap_open, gap_ext in GAPS:
        for match, mismatch in SUBS:
            for read, ref in pairs:
                exp = _oracle(read, ref, match, mismatch, gap_open, gap_ext)
                got = sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K)
                assert got == exp, (shape, gap_open, gap_ext, match, mismatch, bytes(read), bytes(ref), got, exp)


@pytest.mark.parametrize("geo", ((4, 4), (2, 6), (3, 2)), ids=lambda g: "%dx%d" % g)
def test_every_remainder(geo):
    """Reference widths that walk steps % K through 0, 1, ..., K - 1 (and sweeps shorter than one trip), with a read that
    fills the rows and one that leaves `lead` lanes of padding."""
    G, K = geo
    rng = np.random.default_rng(77 + G * K)
    seen = set()
    for R in (G * K, G * K - K - 1 if G > 1 else 1):
        for F in range(1, 2 * K + 2):
            read, ref = _related(rng, R, F)
            for (gap_open, gap_ext), (match, mismatch) in zip(GAPS, SUBS + SUBS):
                exp = _oracle(read, ref, match, mismatch, gap_open, gap_ext)
                assert sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K) == exp, (R, F, gap_open, gap_ext)
            seen.add(_remainder(R, F, G, K))
    assert seen == set(range(K))


def test_one_matching_base_at_every_cell():
    """All mismatches but one matching base at (i, j): only that cell can supply the score -- a lane's last row, the last
    lane, the last column, the lanes above `lead`; its diag + S' sits alone on its anti-diagonal's accumulator."""
    match, mismatch = 2, -1
    for G, K, R in ((4, 4, 16), (4, 4, 13), (4, 4, 5), (3, 2, 6)):
        for F in (5, 6):
            for gap_open, gap_ext in GAPS:
                for i in range(R):
                    for j in range(F):
                        read, ref = np.full(R, ord("A"), dtype=np.uint8), np.full(F, ord("C"), dtype=np.uint8)
                        read[i], ref[j] = ord("G"), ord("G")
                        assert sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K) == match, (G, K, R, F, i, j)


def test_steps_past_the_end_change_nothing():
    """A lane right of column F - 1 only offers values that exist already, tilted or not."""
    rng = np.random.default_rng(5)
    for G, K in ((4, 4), (2, 6)):
        for _ in range(20):
            read, ref = _related(rng, int(rng.integers(1, G * K + 1)), int(rng.integers(1, 12)))
            for extra in (1, K - 1, K):
                assert sweep_score(read, ref, 2, -1, -5, -1, G, K, extra_steps=extra) == _oracle(read, ref, 2, -1, -5, -1)


def test_the_windows_upper_edge():
    """Identical sequences whose last cell drives the largest pattern to exactly 0x7BFF.  Open -5, extend -1, mismatch -1:
    B = 1028.  8 bases on 2 x 4 rows: u reaches rows + F - lead = 16, and 8 x 3837 + 1028 + 16 = 31 740; on 4 x 2 likewise.
    The rule's bound, B + x * u + min(R, F) * match + 1 <= 0x7BFF, is one above what the sweep reaches, as the plain form's is."""
    gap_open, gap_ext, mismatch = -5, -1, -1
    seq = np.frombuffer(b"ACGTTGCA", dtype=np.uint8)
    assert tilt_bias(3837, mismatch, gap_open, gap_ext) == 1028
    for G, K in ((2, 4), (4, 2)):
        top = tilt_top_index(8, 8, G, K)
        assert top == 16
        match = (WINDOW[1] - 1028 - top) // 8
        assert 1028 + top + 8 * match <= WINDOW[1] < 1028 + top + 8 * (match + 1)
        assert sweep_score(seq, seq, match, mismatch, gap_open, gap_ext, G, K) == 8 * match == _oracle(seq, seq, match, mismatch, gap_open, gap_ext)
        with pytest.raises(AssertionError, match="outside the window"):
            sweep_score(seq, seq, match + 1, mismatch, gap_open, gap_ext, G, K)
    # an extension of 3: the tilt takes 3 per unit of u -- 3 x 4 rows, 11 bases, lead 0
    seq11 = np.frombuffer(b"ACGTTGCAGTC", dtype=np.uint8)
    B = tilt_bias(100, -1, -7, -3)
    top = tilt_top_index(11, 11, 3, 4)
    assert B == 1028 and top == 23
    match = (WINDOW[1] - B - 3 * top) // 11
    assert sweep_score(seq11, seq11, match, -1, -7, -3, 3, 4) == 11 * match == _oracle(seq11, seq11, match, -1, -7, -3)
    with pytest.raises(AssertionError, match="outside the window"):
        sweep_score(seq11, seq11, match + 1, -1, -7, -3, 3, 4)


def test_the_windows_edges_are_reached(monkeypatch):
    """The bounds hold and the upper one is reached: no operand lies below B - max(o - x, m), the floor at u = 0 less the most
    a cell can lie below its floor, and the largest pattern sits at u = rows + F - lead: value + B + x * (rows + F - lead)."""
    seen = []
    real = _hmax

    def spy(*patterns):
        seen.extend(patterns)
        return real(*patterns)

    monkeypatch.setattr(sys.modules[__name__], "_hmax", spy)
    read, ref = np.frombuffer(b"ACGTAC", dtype=np.uint8), np.frombuffer(b"TTGCATG", dtype=np.uint8)
    for (gap_open, gap_ext), (match, mismatch) in (((-5, -1), (2, -1)), ((-1, -1), (5, -4)), ((-4, 0), (2, -1)), ((-2, -3), (2, -1))):
        del seen[:]
        sweep_score(read, ref, match, mismatch, gap_open, gap_ext, 3, 2)
        B, o, x, m = tilt_bias(match, mismatch, gap_open, gap_ext), -gap_open, -gap_ext, max(0, -mismatch)
        assert WINDOW[0] <= B - max(o - x, m, 0) <= min(seen)
        if x == 0:                                                   # no tilt: the bound is reached (with x > 0 the first
            assert min(seen) == WINDOW[0]                            # cells sit at u >= 1, up to 2x above it)
    # identical sequences that fill the rows: the last cell is the score, at the largest u
    seq = np.frombuffer(b"ACGTTGCA", dtype=np.uint8)
    del seen[:]
    assert sweep_score(seq, seq, 7, -1, -5, -2, 2, 4) == 56
    assert max(seen) == tilt_bias(7, -1, -5, -2) + 2 * tilt_top_index(8, 8, 2, 4) + 56
