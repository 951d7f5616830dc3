"""The int16 Smith-Waterman sweep with symmetric affine gaps, restated on the CPU (no GPU, no HIP code involved): per cell it
carries the best SOURCE of a gap instead of the gap's score -- XE(q, j) = max over earlier columns k of H(q, k) - (j - 1 - k) ext,
XF likewise down the column -- so that E = XE - open, F = XF - open and

    g = max(XE, XF);  h = max(diag + S, g - open);  XE' = max(XE - ext, h);  XF' = max(XF - ext, h)      (every "-" floored at 0)

is the Gotoh cell in 9 packed instructions per register, and g, which is at least the cell to the left and the cell above and
never more than a cell that exists, feeds the running maximum once per pair of steps (Recurrences and Tracking).
This file runs the sweep as score_kernel runs it, with plain Python loops: lane groups of G lanes with K rows each, rows
padded at the top, the sweep started `lead` lanes down, unmasked steps before column 0 and after column F - 1, steps in pairs
(the first tracks nothing, the second every g plus its last h) and the leftover step of an odd count tracking diag + S.  The
scores are compared with oracle.cpu_ref.score over the scorings of tests/test_gpu_sym_affine_sweep.py."""
import numpy as np
import pytest

from oracle import cpu_ref

_CLASS = {ord(c): k for k, cs in ((1, "Aa"), (2, "Tt"), (3, "Cc"), (4, "Gg"), (5, "Nn")) for c in cs}      # DefaultKernel.h:43-60

GAPS = ((-5, -1), (-1, -1), (-2, -3), (-4, 0), (0, 0))          # (open, extend): open above, equal to and below extend, free gaps
SUBS = ((2, -1), (5, -4))
GEOMETRIES = ((1, 1), (2, 1), (1, 3), (2, 2), (3, 2), (4, 3), (8, 2), (5, 4))      # (G, K) of the model: any lane count will do


def _sub(a, b, match, mismatch):
    ca, cb = _CLASS.get(int(a), 0), _CLASS.get(int(b), 0)
    if 1 <= ca <= 4 and 1 <= cb <= 4:
        return match if ca == cb else mismatch
    return 0


def _floor0(a, g):
    """pk_sub_floor0: an unsigned saturating subtract of a magnitude from a non-negative cell."""
    assert a >= 0 and g >= 0
    return max(a - g, 0)


def sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K):
    R, F = len(read), len(ref)
    rows = G * K
    assert R <= rows
    o, e = -gap_open, -gap_ext
    S = np.zeros((rows, F), dtype=np.int64)                         # rows padded at the top score nothing
    for r in range(R):
        for j in range(F):
            S[rows - R + r, j] = _sub(read[r], ref[j], match, mismatch)
    lead = (rows - R) // K if rows > R else 0
    Hl = [[0] * K for _ in range(G)]
    XE = [[0] * K for _ in range(G)]
    up0, h_last, f_last, best = [0] * G, [0] * G, [0] * G, [0] * G

    def step(t, track):
        h_in = [0] + h_last[:-1]                                      # what the lane above held before this step; border: 0
        f_in = [0] + f_last[:-1]
        for l in range(G):
            j = t - l + lead                                          # lanes outside [0, F) read the zero slab, unmasked
            s = S[l * K:(l + 1) * K, j] if 0 <= j < F else np.zeros(K, dtype=np.int64)
            diag0, up0[l] = up0[l], h_in[l]
            xf, d, h = f_in[l], diag0 + int(s[0]), 0
            for q in range(K):
                g = max(XE[l][q], xf)
                d_next = Hl[l][q] + int(s[q + 1]) if q + 1 < K else 0
                a, y, b = _floor0(XE[l][q], e), _floor0(g, o), _floor0(xf, e)
                if track == "all":
                    best[l] = max(best[l], d)
                elif track == "pair":
                    best[l] = max(best[l], g)
                h = max(d, y)
                Hl[l][q], XE[l][q], xf, d = h, max(a, h), max(b, h), d_next
            if track == "pair":
                best[l] = max(best[l], h)
            h_last[l], f_last[l] = h, xf

    steps = F + G - 1 - lead
    t = 0
    while t + 1 < steps:
        step(t, "none")
        step(t + 1, "pair")
        t += 2
    if t < steps:
        step(t, "all")
    return max(best)


def _case(rng):
    G, K = GEOMETRIES[int(rng.integers(0, len(GEOMETRIES)))]
    R = int(rng.integers(1, G * K + 1))
    F = int(rng.integers(1, 15))
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
    return G, K, read, ref


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("gaps", GAPS)
def test_gap_source_sweep_is_the_oracle(gaps, sub):
    rng = np.random.default_rng(1000 * GAPS.index(gaps) + SUBS.index(sub))
    (gap_open, gap_ext), (match, mismatch) = gaps, sub
    sc = cpu_ref.Scoring.make(match, mismatch, -3, -3, gap_open, gap_ext, gap_open, gap_ext)
    parities = set()
    for case in range(300):
        G, K, read, ref = _case(rng)
        exp = int(cpu_ref.score(0, read[None, :], ref[None, :], sc, affine=True)[0])
        got = sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K)
        assert got == exp, (case, G, K, bytes(read), bytes(ref), got, exp)
        parities.add((len(ref) + G - 1) % 2)
    assert parities == {0, 1}


def test_one_matching_base_at_every_cell():
    """All mismatches but one matching base at (i, j): only that cell can supply the score -- the last row of a lane on a
    first and on a second step, the last lane, the last column, the leftover step, the lanes above `lead`."""
    match, mismatch = 2, -1
    for G, K, R in ((4, 3, 12), (4, 3, 11), (4, 3, 5), (3, 2, 6)):
        for F in (5, 6):
            for gap_open, gap_ext in GAPS:
                for i in range(R):
                    for j in range(F):
                        read, ref = np.full(R, ord("A"), dtype=np.uint8), np.full(F, ord("C"), dtype=np.uint8)
                        read[i], ref[j] = ord("G"), ord("G")
                        assert sweep_score(read, ref, match, mismatch, gap_open, gap_ext, G, K) == match, (G, K, R, F, i, j)
