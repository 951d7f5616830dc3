"""The row-table step of the tilted int16 Smith-Waterman sweep with symmetric affine gaps (dp_kernels.hip.h: tilted_step, forms
kRowTables / kRowTablesRepair) with its adds and its subtract done ON THE 32-BIT WORD that holds pair A in the low and pair B in
the high half -- d = diag + S', ho = h - (o - x), the two slot adds acc[slot] + K x and fl[slot] + K x, lead_border + lead_step --
restated on the CPU (no GPU, no HIP code involved), in the manner of tests/test_sym_affine_row_tables_sweep.py and
tests/test_sym_affine_odd_tile_sweep.py: the same cell, hand-over, floors, accumulators, rotation, plain and repairing form,
even and odd K, but on BOTH pairs of a register at once.

The restatement runs twice: `halves` adds and subtracts each half by itself and wraps at 16 bits (v_pk_add_u16 / v_pk_sub_i16),
`word` is one uint32 add or subtract of the packed pair (v_add_u32 / v_sub_u32).  Asserted:

  * every register of every lane is equal after every step, and so is the score of both pairs, which is the oracle's;
  * no half of an operand of those adds leaves the bounds the kernel's comment states -- S' in [0, 255], o - x in [0, 255],
    diag, d, h, ho, acc, fl and the border in [0x0400, 0x7BFF], the sums of the slot adds below 0x10000, the masked halves of
    lead_border and lead_step 0 -- so no half carries or borrows into its neighbour.

Pairs are built so that one half is at its largest while the other is at its floor, and the other way round: a long perfect
match (the read is the reference's last R bases) beside a pair of mismatches only, or beside an empty reference.

The diagonal is the one the kernel takes: d[q] = HOl[q - 1] + S''[q], H - (o - x) of the row above as it was one step earlier,
with o - x riding on EVERY row's table bytes (`ho_diagonal`; row 0 takes the handed-over ho as before) -- no H register is kept.
That form is compared with oracle.cpu_ref.score, not with itself; the H-register form it replaces runs beside it.

The mutant: with table values that may be negative -- the LDS-profile form's S', e.g. mismatch -3 with extend -1 -- the word form
differs from the halves form and from the oracle (a negative half is 0xFFFF.. and carries into its neighbour); the kernel keeps
its packed instructions there."""
import numpy as np
import pytest

import test_sym_affine_tilted_sweep as frame
from test_sym_affine_row_tables_sweep import REPAIR, TABLES, last_acgt_end, needs_repair, rule_ok
from test_sym_affine_tilted_sweep import WINDOW, _CLASS, _HALF, _oracle, tilt_bias, tilt_top_index

HALVES, WORD = "halves", "word"
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
BENCH = (2, -1, -5, -1)
X_ZERO = (3, 1, -4, 0)                  # x = 0: no tilt, every floor is B
OX_ZERO = (2, -1, -1, -1)               # o - x = 0: the subtract takes nothing off
BYTE_255 = (249, -1, -5, -1)            # the largest table byte, match' + (o - x), is exactly 255
NEGATIVE = (2, -3, -5, -1)              # mismatch' = -1: no byte; the LDS-profile form's case
# shape x scoring whose largest operand is exactly 0x7BFF: B + x * top + min(R, F) * match, the full score in the last cell.
# (sym_affine_tilt_ok keeps one spare unit and stops at 0x7BFE -- EDGE_RULE below, the last scoring it admits; the window and
# the no-carry argument hold up to 0x7BFF itself.)
EDGE_TOP = {(8, 19): (152, 152, (2, -1, -115, -100)), (16, 10): (160, 165, (1, -1, -103, -94))}
EDGE_RULE = {(8, 19): (152, 152, (2, -1, -114, -100)), (16, 10): (160, 165, (1, -1, -102, -94))}


def pack(lo, hi):
    assert 0 <= lo <= 0xFFFF and 0 <= hi <= 0xFFFF
    return lo | hi << 16


def halves(w):
    return w & 0xFFFF, w >> 16


class Bounds:
    """Smallest and largest half of every named operand"""

    def __init__(self):
        self.lo, self.hi = {}, {}

    def see(self, name, word):
        for v in halves(word):
            if v < self.lo.get(name, 1 << 20):
                self.lo[name] = v
            if v > self.hi.get(name, -1):
                self.hi[name] = v

    def check(self, ox, kx):
        """The bounds of dp_kernels.hip.h's WORD ARITHMETIC paragraph, operand by operand"""
        lo, hi = self.lo, self.hi
        assert 0 <= lo["S"] and hi["S"] <= 255, (lo["S"], hi["S"])                                    # sym_affine_row_tables_ok
        for name in ("diag", "d", "h", "ho", "acc", "fl", "border"):                                  # the window
            assert WINDOW[0] <= lo[name] and hi[name] <= WINDOW[1], (name, hex(lo[name]), hex(hi[name]))
        assert 0 <= ox <= 255 and 0 <= kx
        assert hi["acc+kx"] <= 0xFFFF and hi["fl+kx"] <= 0xFFFF and hi["fl+kx"] <= WINDOW[1] + kx
        assert lo.get("masked", 0) == hi.get("masked", 0) == 0                                        # (a one-lane group has none)


def _hmax_w(bounds_ok, *words):
    """v_pk_maximum3_f16 / v_pk_maximum_f16 on patterns of the window: per half"""
    out = 0
    for shift in (0, 16):
        ps = [(w >> shift) & 0xFFFF for w in words]
        if bounds_ok:
            for p in ps:
                assert WINDOW[0] <= p <= WINDOW[1], ("operand outside the window", hex(p))
        out |= max(ps, key=_HALF.__getitem__) << shift
    return out


def _fmax_w(bounds_ok, f, ho):
    """max(f, ho) where f may be the +0.0 a lane shift delivers in a group's first lane"""
    if f == 0:
        return _hmax_w(bounds_ok, ho)
    return _hmax_w(bounds_ok, f, ho)


def sweep(pair_a, pair_b, scoring, G, K, mode, form=None, ho_diagonal=True, cols=None, profile_scores=False, trace=None, bounds=None):
    """Both pairs of a register through the row-table sweep -> (score A, score B).  mode: HALVES or WORD.  form: TABLES / REPAIR
    (None: what the wave would run).  ho_diagonal: the diagonal from HOl with o - x on every row's table (else from Hl, o - x on
    row 0's).  profile_scores: S' as 16-bit two's complement values that may be negative (the LDS-profile form's: the mutant).
    trace: a list that receives every register after every step."""
    match, mismatch, gap_open, gap_ext = scoring
    (read_a, ref_a), (read_b, ref_b) = pair_a, pair_b
    R = len(read_a)
    assert len(read_b) == R and len(ref_a) == len(ref_b)
    rows = G * K
    assert R <= rows and (profile_scores or rule_ok(*scoring))
    o, x = -gap_open, -gap_ext
    ox, kx = o - x, K * x
    B = tilt_bias(*scoring)
    end = max(last_acgt_end(ref_a), last_acgt_end(ref_b))
    F = end if cols is None else cols                                 # the wave's cols_used
    assert F >= end
    if form is None:
        form = REPAIR if needs_repair(ref_a[:F]) or needs_repair(ref_b[:F]) else TABLES
    checked = not profile_scores                                     # (the mutant leaves the window: nothing is asserted of it)

    def add(a, b):
        if mode == WORD:
            return (a + b) & 0xFFFFFFFF
        return pack((a + b) & 0xFFFF, ((a >> 16) + (b >> 16)) & 0xFFFF)

    def sub(a, b):
        if mode == WORD:
            return (a - b) & 0xFFFFFFFF
        return pack((a - b) & 0xFFFF, ((a >> 16) - (b >> 16)) & 0xFFFF)

    def both(v):
        return pack(v & 0xFFFF, v & 0xFFFF)

    def table(read):
        T = []
        for p in range(rows):
            a = _CLASS.get(int(read[p - (rows - R)]), 0) if p >= rows - R else 0
            row = [(match if a == c else mismatch) + 2 * x if 1 <= a <= 4 else 2 * x for c in (1, 2, 3, 4)]
            row = [v + (ox if ho_diagonal or p % K == 0 else 0) for v in row]
            assert profile_scores or all(0 <= v <= 255 for v in row), row
            T.append(row)
        return T

    Ta, Tb = table(read_a), table(read_b)
    zero_fix = [2 * x + (ox if ho_diagonal or q == 0 else 0) for q in range(K)]

    def sel(ref, j):
        c = _CLASS.get(int(ref[j]), 0) if 0 <= j < len(ref) and j < F else 0
        return c - 1 if 1 <= c <= 4 else None

    def score(l, q, j):
        out = 0
        for shift, T, ref in ((0, Ta, ref_a), (16, Tb, ref_b)):
            c = sel(ref, j)
            s = T[l * K + q][c] if c is not None else (zero_fix[q] if form == REPAIR or profile_scores else 0)
            out |= (s & 0xFFFF) << shift
        return out

    lead = (rows - R) // K if rows > R else 0
    steps = F + G - 1 - lead

    def u_of(l, q, t):
        return l * (K - 1) + q + t + 2

    ox_c, kx_c = both(ox), both(kx)
    Hl = [[both(B + x * u_of(l, q, -1)) for q in range(K)] for l in range(G)]
    El = [list(row) for row in Hl]
    HOl = [[sub(v, ox_c) for v in row] for row in Hl]
    up0 = [both(B + x * u_of(l, -1, -1) - ox) for l in range(G)]
    f_last = [HOl[l][K - 1] for l in range(G)]
    s0 = K - steps % K
    fl = [[both(B + x * u_of(l, (i - s0) % K, 0)) for i in range(K)] for l in range(G)]
    acc = [list(row) for row in fl]
    dprev = [[both(B + x * u_of(l, q - 1, 0)) if q & 1 else None for q in range(K)] for l in range(G)]
    # the moving border: in the group's first lane only, 0 (both halves) in every other
    lead_border = [both(B + x * u_of(0, -1, 0) - ox)] + [0] * (G - 1)
    lead_step = [both(x)] + [0] * (G - 1)
    see = bounds.see if bounds is not None else (lambda name, word: None)

    def step(t, s):
        h_in = [0 | lead_border[0]] + [HOl[l][K - 1] | lead_border[l + 1] for l in range(G - 1)]
        f_in = [0] + f_last[:-1]
        for l in range(G):
            j = t - l + lead
            diag0, up0[l] = up0[l], h_in[l]
            see("border" if l == 0 else "masked", lead_border[l])
            see("masked" if l else "step", lead_step[l])
            lead_border[l] = add(lead_border[l], lead_step[l])
            left = list(HOl[l]) if ho_diagonal else list(Hl[l])
            f, ho = f_in[l], up0[l]
            ds = []
            for q in range(K):
                floor = fl[l][(q + s) % K]
                assert floor == both(B + x * u_of(l, q, t))
                diag, S = diag0 if q == 0 else left[q - 1], score(l, q, j)
                d = add(diag, S)
                e = _hmax_w(checked, El[l][q], HOl[l][q], floor)
                f = _fmax_w(checked, f, ho)
                h = _hmax_w(checked, d, e, f)
                ho = sub(h, ox_c)
                for name, word in (("diag", diag), ("S", S), ("d", d), ("h", h), ("ho", ho)):
                    see(name, word)
                Hl[l][q], El[l][q], HOl[l][q] = h, e, ho
                ds.append(d)
            f_last[l] = f
            a = acc[l]
            for q in range(0, K, 2):
                slot = (q + s) % K
                a[slot] = _hmax_w(checked, a[slot], ds[q], dprev[l][q + 1]) if q + 1 < K else _hmax_w(checked, a[slot], ds[q])
            for q in range(1, K, 2):
                dprev[l][q] = ds[q]
            see("acc", a[s])
            see("fl", fl[l][s])
            a[s] = add(a[s], kx_c)
            fl[l][s] = add(fl[l][s], kx_c)
            see("acc+kx", a[s])
            see("fl+kx", fl[l][s])
        if trace is not None:
            regs = (HOl, El, acc, fl, dprev, [up0], [f_last], [lead_border]) + (() if ho_diagonal else (Hl,))
            trace.append(tuple(tuple(v for row in reg for v in row) for reg in regs))

    t = 0
    for s in range(s0 % K, K if s0 < K else 0):
        step(t, s)
        t += 1
    while t < steps:
        for s in range(K):
            step(t, s)
            t += 1
    assert t == steps
    best = [0, 0]
    for l in range(G):
        for q in range(0, K - 1, 2):
            acc[l][q] = _hmax_w(checked, acc[l][q], dprev[l][q + 1])
        for slot in range(K):
            # out of the frame: a packed subtract in both forms (v_pk_sub_i16; the difference may be anything)
            for i, (av, fv) in enumerate(zip(halves(acc[l][slot]), halves(fl[l][slot]))):
                best[i] = max(best[i], frame._i16((av - fv) & 0xFFFF))
    if bounds is not None and checked:
        bounds.check(ox, kx)
    return tuple(best)


# ---- the pairs: one half at its largest while the other is at its floor ----
def perfect(R, F, seed):
    """The read is the reference's last R bases: the full score lands in the last row at the last column, the largest u"""
    rng = np.random.default_rng(seed)
    ref = ACGT[rng.integers(0, 4, size=F)].copy()
    return ref[F - min(R, F):].copy() if R <= F else np.concatenate((ACGT[rng.integers(0, 4, size=R - F)], ref)), ref


def mismatches(R, F):
    return np.full(R, ord("A"), dtype=np.uint8), np.full(F, ord("C"), dtype=np.uint8)


def empty(R, F):
    return np.full(R, ord("G"), dtype=np.uint8), np.zeros(F, dtype=np.uint8)


def hazard_pairs(R, F, seed):
    """[(name, pair A, pair B)]: the long match in the low half, then in the high half; its partner scores nothing"""
    hot = perfect(R, F, seed)
    out = []
    for name, cold in (("mismatches", mismatches(R, F)), ("empty", empty(R, F))):
        out += [("match|" + name, hot, cold), (name + "|match", cold, hot)]
    return out


def both_ways(pair_a, pair_b, scoring, G, K, **kw):
    """halves and word: every register after every step, the scores and the bounds -> the scores"""
    runs = {}
    for mode in (HALVES, WORD):
        trace, bounds = [], Bounds()
        runs[mode] = (sweep(pair_a, pair_b, scoring, G, K, mode, trace=trace, bounds=bounds, **kw), trace, bounds)
    (sc_h, tr_h, b_h), (sc_w, tr_w, b_w) = runs[HALVES], runs[WORD]
    assert len(tr_h) == len(tr_w) > 0
    for t, (a, b) in enumerate(zip(tr_h, tr_w)):
        assert a == b, ("registers differ after step", t)
    assert sc_h == sc_w and (b_h.lo, b_h.hi) == (b_w.lo, b_w.hi)
    return sc_w, b_w


TILES = ((8, 19), (16, 10))
SHAPES = {(8, 19): ((150, 27), (129, 20)), (16, 10): ((150, 21), (160, 14))}


@pytest.mark.parametrize("scoring", (BENCH, X_ZERO, OX_ZERO, BYTE_255), ids=("bench", "x0", "ox0", "byte255"))
@pytest.mark.parametrize("tile", TILES, ids=lambda g: "%dx%d" % g)
def test_word_arithmetic_is_the_packed_arithmetic(tile, scoring):
    G, K = tile
    assert rule_ok(*scoring) and (scoring != BYTE_255 or max(scoring[:2]) - 2 * scoring[3] + scoring[3] - scoring[2] == 255)
    for R, F in SHAPES[tile]:
        for name, pair_a, pair_b in hazard_pairs(R, F, seed=R + F):
            exp = (_oracle(*pair_a, *scoring), _oracle(*pair_b, *scoring))
            cold = min(R, F) * max(scoring[1], 0) if "mismatches" in name else 0      # (a mismatch score above zero: X_ZERO)
            assert sorted(exp) == [cold, min(R, F) * scoring[0]], (name, exp)
            got, bounds = both_ways(pair_a, pair_b, scoring, G, K, cols=F + 2)
            assert got == exp, (tile, scoring, R, F, name, got, exp)
            assert bounds.hi["S"] == max(scoring[:2]) - 2 * scoring[3] + scoring[3] - scoring[2]      # match' + (o - x) was added


@pytest.mark.parametrize("tile", TILES, ids=lambda g: "%dx%d" % g)
def test_the_repairing_form_and_bases_that_score_nothing(tile):
    G, K = tile
    R, F = SHAPES[tile][0]
    hot, cold = perfect(R, F, seed=3), mismatches(R, F)
    dirty = (hot[0], hot[1].copy())
    dirty[1][F // 2] = ord("N")                                       # before the last ACGT base: the wave repairs
    assert needs_repair(dirty[1])
    all_n = (hot[0], np.full(F, ord("N"), dtype=np.uint8))
    for pair_a, pair_b in ((dirty, cold), (cold, dirty), (dirty, empty(R, F)), (all_n, hot), (hot, all_n), (empty(R, F), all_n)):
        exp = (_oracle(*pair_a, *BENCH), _oracle(*pair_b, *BENCH))
        got, _ = both_ways(pair_a, pair_b, BENCH, G, K, cols=F + 1)
        assert got == exp, (tile, got, exp)
    # a clean wave through the repairing copy of the step
    got, _ = both_ways(hot, cold, BENCH, G, K, form=REPAIR)
    assert got == (_oracle(*hot, *BENCH), 0)


@pytest.mark.parametrize("tile", TILES, ids=lambda g: "%dx%d" % g)
def test_the_windows_upper_edge(tile):
    """Largest operand exactly 0x7BFF (one past the rule's spare unit) and exactly 0x7BFE (the last scoring the rule admits)"""
    G, K = tile
    for table, top_pattern in ((EDGE_TOP, WINDOW[1]), (EDGE_RULE, WINDOW[1] - 1)):
        R, F, scoring = table[tile]
        B, x, top = tilt_bias(*scoring), -scoring[3], tilt_top_index(R, F, G, K)
        assert rule_ok(*scoring) and B + x * top + min(R, F) * scoring[0] == top_pattern
        for name, pair_a, pair_b in hazard_pairs(R, F, seed=F)[:2]:
            exp = (_oracle(*pair_a, *scoring), _oracle(*pair_b, *scoring))
            got, bounds = both_ways(pair_a, pair_b, scoring, G, K)
            assert got == exp and sorted(exp) == [0, min(R, F) * scoring[0]], (name, got, exp)
            assert max(bounds.hi[k] for k in ("d", "h", "acc")) == top_pattern, (name, hex(bounds.hi["h"]))
            assert bounds.lo["ho"] >= WINDOW[0] and bounds.hi["acc+kx"] < 0x10000


def test_the_h_register_form_agrees():
    """What the step did before: diagonals from Hl, o - x on row 0's table alone.  Same scores, word or halves."""
    for G, K in TILES:
        R, F = SHAPES[(G, K)][0]
        for name, pair_a, pair_b in hazard_pairs(R, F, seed=1)[:2]:
            exp = (_oracle(*pair_a, *BENCH), _oracle(*pair_b, *BENCH))
            got, _ = both_ways(pair_a, pair_b, BENCH, G, K, ho_diagonal=False, cols=F + 3)
            assert got == exp


def test_random_pairs_on_small_tiles():
    rng = np.random.default_rng(29)
    for case in range(60):
        G, K = ((2, 3), (3, 4), (2, 5), (4, 2), (1, 7))[case % 5]
        R, F = int(rng.integers(1, G * K + 1)), int(rng.integers(1, 14))
        scoring = (BENCH, X_ZERO, OX_ZERO, (5, -2, -7, -1))[case % 4]
        pairs = []
        for _ in range(2):
            read, ref = frame._related(rng, R, F)
            pairs.append((read, ref))
        exp = tuple(_oracle(*p, *scoring) for p in pairs)
        got, _ = both_ways(pairs[0], pairs[1], scoring, G, K, cols=F + case % 3)
        assert got == exp, (G, K, R, F, scoring, got, exp)


def test_negative_table_values_break_the_word_form():
    """The mutant.  S' = mismatch + 2x = -1 is 0xFFFF in its half: on the word it carries into the neighbour (or, in the high
    half, out of the register), which is why the LDS-profile form keeps v_pk_add_u16.  The halves form stays the oracle."""
    assert not rule_ok(*NEGATIVE)
    for G, K in TILES:
        R, F = SHAPES[(G, K)][0]
        cold, hot = mismatches(R, F), perfect(R, F, seed=5)
        exp = (_oracle(*cold, *NEGATIVE), _oracle(*hot, *NEGATIVE))
        tr_h, tr_w = [], []
        got_h = sweep(cold, hot, NEGATIVE, G, K, HALVES, ho_diagonal=False, profile_scores=True, trace=tr_h)
        got_w = sweep(cold, hot, NEGATIVE, G, K, WORD, ho_diagonal=False, profile_scores=True, trace=tr_w)
        assert got_h == exp
        assert tr_h != tr_w and got_w != exp, (got_w, exp)
        # ... and the bounds say so before any score does
        bounds = Bounds()
        sweep(cold, hot, NEGATIVE, G, K, HALVES, ho_diagonal=False, profile_scores=True, bounds=bounds)
        with pytest.raises(AssertionError):
            bounds.check(4, K)


def test_the_restatement_can_fail():
    """A word subtract that borrows: were o - x allowed above the smallest h (it is not: B >= 1024 + o - x), the halves would
    part.  Shown on the helper the sweep uses, with a register at its floor beside one above it."""
    h = pack(0x0400, 0x0500)
    ox = pack(0x0401, 0x0401)
    word, per_half = (h - ox) & 0xFFFFFFFF, pack((0x0400 - 0x0401) & 0xFFFF, (0x0500 - 0x0401) & 0xFFFF)
    assert word != per_half and halves(word)[1] == halves(per_half)[1] - 1
    # ... and an add that carries: a table value of 0xFFFF (-1) in the low half
    d_word, d_half = (pack(0x0400, 0x0400) + pack(0xFFFF, 0)) & 0xFFFFFFFF, pack(0x03FF, 0x0400)
    assert d_word != d_half and halves(d_word) == (0x03FF, 0x0401)
