"""The biased form of the int16 Smith-Waterman sweep with symmetric affine gaps, restated on the CPU (no GPU, no HIP code
involved).  Every cell is kept as value + B with B = 1024 + o + x + m (o = -open, x = -extend, m = the most a substitution
score takes off a cell), adds and subtracts are plain 16-bit ones that wrap, and every maximum is taken ON THE BIT PATTERNS
READ AS HALF FLOATS, as gfx950's v_pk_maximum3_f16 takes it:

    d = diag + S;  e = max3(E - ext, HO, B);  f = max(f - ext, ho);  h = max3(d, e, f);  ho = h - open

That is an integer maximum exactly while every operand lies in [0x0400, 0x7BFF], the positive normal halves, and this file
asserts that of every operand of every maximum (Recurrences: the window).  The sweep runs as score_kernel runs it,
with plain Python loops: lane groups of G lanes with K rows each, rows padded at the top, the sweep started `lead` lanes
down, unmasked steps before column 0 and after column F - 1, every border at B, the running maximum fed with diag + S two rows
at a time.  The scores are compared with oracle.cpu_ref.score over the scorings of tests/test_gpu_sym_affine_sweep.py plus
a positive mismatch score, at fixed shapes and random ones, and at the window's upper edge."""
import numpy as np
import pytest

from oracle import cpu_ref

_CLASS = {ord(c): k for k, cs in ((1, "Aa"), (2, "Tt"), (3, "Cc"), (4, "Gg"), (5, "Nn")) for c in cs}      # DefaultKernel.h:43-60

GAPS = ((-5, -1), (-1, -1), (-2, -3), (-4, 0), (0, 0))          # (open, extend) of tests/test_gpu_sym_affine_sweep.py
SUBS = ((2, -1), (5, -4), (3, 1))                               # ... its substitution scores, and a positive mismatch score
GEOMETRIES = ((1, 2), (2, 2), (1, 4), (3, 2), (4, 4), (8, 2), (5, 4), (2, 1), (3, 3))      # (G, K) of the model (odd K: the last even row)

WINDOW = (0x0400, 0x7BFF)
# the value of every 16-bit pattern read as a half float (NaNs included: a pattern outside the window fails its assertion first)
_HALF = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float64).tolist()


def _sub(a, b, match, mismatch):
    ca, cb = _CLASS.get(int(a), 0), _CLASS.get(int(b), 0)
    if 1 <= ca <= 4 and 1 <= cb <= 4:
        return match if ca == cb else mismatch
    return 0


def _add16(a, b):
    """v_pk_add_u16 / v_pk_sub_i16 without a clamp: 16 bits, wraps."""
    return (a + b) & 0xFFFF


def _hmax(*patterns):
    """A half-float maximum of bit patterns, every operand inside the window."""
    for p in patterns:
        assert WINDOW[0] <= p <= WINDOW[1], ("operand outside the window", hex(p))
    return max(patterns, key=_HALF.__getitem__)


def bias(match, mismatch, gap_open, gap_ext):
    return 1024 - gap_open - gap_ext + max(0, -mismatch, -match)


def sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K):
    R, F = len(read), len(ref)
    rows = G * K
    assert R <= rows
    o, x = -gap_open, -gap_ext
    B = bias(match, mismatch, gap_open, gap_ext)
    S = np.zeros((rows, F), dtype=np.int64)                         # rows padded at the top score nothing
    for r in range(R):
        for j in range(F):
            S[rows - R + r, j] = _sub(read[r], ref[j], match, mismatch)
    lead = (rows - R) // K if rows > R else 0
    Hl = [[B] * K for _ in range(G)]
    El = [[B] * K for _ in range(G)]
    HOl = [[_add16(B, -o)] * K for _ in range(G)]
    up0, h_last, f_last, best = [B] * G, [B] * G, [B] * G, [B] * G

    def step(t):
        h_in = [B] + h_last[:-1]                                      # what the lane above held before this step; border: B
        f_in = [B] + f_last[:-1]
        for l in range(G):
            j = t - l + lead                                          # lanes outside [0, F) read the zero slab, unmasked
            s = S[l * K:(l + 1) * K, j] if 0 <= j < F else np.zeros(K, dtype=np.int64)
            diag0, up0[l] = up0[l], h_in[l]
            left = list(Hl[l])                                        # H of the previous column
            f, ho, d_prev = f_in[l], _add16(up0[l], -o), None
            for q in range(K):
                d = _add16(diag0 if q == 0 else left[q - 1], int(s[q]))
                e = _hmax(_add16(El[l][q], -x), HOl[l][q], B)
                f = _hmax(_add16(f, -x), ho)
                h = _hmax(d, e, f)
                ho = _add16(h, -o)
                Hl[l][q], El[l][q], HOl[l][q] = h, e, ho
                if q & 1:
                    best[l] = _hmax(best[l], d_prev, d)
                elif q == K - 1:
                    best[l] = _hmax(best[l], d)
                d_prev = d
            h_last[l], f_last[l] = h, f

    for t in range(F + G - 1 - lead):
        step(t)
    res = max(_add16(b, -B) for b in best)                            # all >= 0: best >= B
    assert res < 0x8000
    return res


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


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("gaps", GAPS)
def test_biased_sweep_is_the_oracle(gaps, sub):
    rng = np.random.default_rng(2000 * GAPS.index(gaps) + SUBS.index(sub))
    (gap_open, gap_ext), (match, mismatch) = gaps, sub
    parities = set()
    for case in range(200):
        G, K = GEOMETRIES[int(rng.integers(0, len(GEOMETRIES)))]
        read, ref = _related(rng, int(rng.integers(1, G * K + 1)), int(rng.integers(1, 15)))
        exp = _oracle(read, ref, match, mismatch, gap_open, gap_ext)
        got = sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K)
        assert got == exp, (case, G, K, bytes(read), bytes(ref), got, exp)
        parities.add((len(ref) + G - 1) % 2)
    assert parities == {0, 1}


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


def test_one_matching_base_at_every_cell():
    """All mismatches but one matching base at (i, j): only that cell can supply the score -- a lane's last row, the last
    lane, the last column, the lanes above `lead`."""
    match, mismatch = 2, -1
    for G, K, R in ((4, 4, 16), (4, 4, 13), (4, 4, 5), (3, 2, 6)):
        for F in (5, 6):
            for gap_open, gap_ext in GAPS:
                for i in range(R):
                    for j in range(F):
                        read, ref = np.full(R, ord("A"), dtype=np.uint8), np.full(F, ord("C"), dtype=np.uint8)
                        read[i], ref[j] = ord("G"), ord("G")
                        assert sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K) == match, (G, K, R, F, i, j)


def test_the_windows_upper_edge():
    """Identical sequences whose score drives the largest pattern to exactly 0x7BFF: open -5, extend -1, mismatch -1 give
    B = 1031, and 8 bases at 3839 a match score 30 712 = 0x7BFF - 1031.  One more and a maximum is handed +inf's pattern."""
    gap_open, gap_ext, mismatch = -5, -1, -1
    seq = np.frombuffer(b"ACGTTGCA", dtype=np.uint8)
    assert bias(3839, mismatch, gap_open, gap_ext) == 1031 and 1031 + 8 * 3839 == WINDOW[1]
    for G, K in ((2, 4), (4, 2), (3, 4)):
        got = sweep_score(seq, seq, 3839, mismatch, gap_open, gap_ext, G, K)
        assert got == 8 * 3839 == _oracle(seq, seq, 3839, mismatch, gap_open, gap_ext)
    seq11 = np.frombuffer(b"ACGTTGCAGTC", dtype=np.uint8)           # 11 x 2792 = 30 712 as well: an odd length, other rows
    assert sweep_score(seq11, seq11, 2792, mismatch, gap_open, gap_ext, 3, 4) == 30712 == _oracle(seq11, seq11, 2792, mismatch, gap_open, gap_ext)
    with pytest.raises(AssertionError, match="outside the window"):
        sweep_score(seq11, seq11, 2793, mismatch, gap_open, gap_ext, 3, 4)      # 1031 + 30 723 > 0x7BFF


def test_the_windows_lower_edge(monkeypatch):
    """The bounds of the window proof are reached, not merely respected: the smallest operand a sweep hands a maximum is the
    extension of a fresh gap below the border, B - o - x, or a mismatch on the border, B - m."""
    import sys
    seen = []
    real = _hmax

    def spy(*patterns):
        seen.extend(patterns)
        return real(*patterns)

    monkeypatch.setattr(sys.modules[__name__], "_hmax", spy)
    read, ref = np.frombuffer(b"ACGTAC", dtype=np.uint8), np.frombuffer(b"TTGCATG", dtype=np.uint8)
    for (gap_open, gap_ext), (match, mismatch) in (((-5, -1), (2, -1)), ((-1, -1), (5, -4)), ((-4, 0), (2, -1))):
        del seen[:]
        sweep_score(read, ref, match, mismatch, gap_open, gap_ext, 3, 2)
        B, o, x, m = bias(match, mismatch, gap_open, gap_ext), -gap_open, -gap_ext, max(0, -mismatch)
        assert min(seen) == min(B - o - x, B - m) >= WINDOW[0]
