"""tests/extend_band_ref.py against what it must agree with, on the CPU: with B = 1 a brute-force plain-Python fill of the per-cell
band |i - j| <= w; with w >= max(R, F) tests/extend_ref.py exactly; per-cell band <= block band <= unbanded for score and gscore
(an unreached read end counts as minus infinity); and the closed form of the unreached read end against "row Rp - 1 has no
present candidate" on an exhaustive small grid."""
import numpy as np
import pytest

import extend_band_ref as ebr
import extend_ref
from versalignlib_amd import hipkernel

FORMS = {"sym": (-3, -3), "lin": (-2, -4), "affsym": (-3, -3, -5, -1, -5, -1), "aff": (-3, -3, -6, -2, -4, -1)}
BASES = np.frombuffer(b"ACGT", np.uint8)


def _scoring(form):
    return hipkernel.Scoring.make(2, -1, *FORMS[form])


def _pairs(n, R, F, seed):
    """reads against references that share a prefix, some with extra reference bases, some trimmed"""
    rng = np.random.default_rng(seed)
    reads, refs = BASES[rng.integers(0, 4, (n, R))], BASES[rng.integers(0, 4, (n, F))]
    for p in range(n):
        L = int(rng.integers(1, min(R, F) + 1))
        d = int(rng.integers(0, 4)) if p % 2 else 0
        refs[p, d:d + min(L, F - d)] = reads[p, :min(L, F - d)]
        if p % 3 == 0:
            reads[p, int(rng.integers(1, R + 1)):] = ord("N")
        if p % 4 == 1:
            refs[p, int(rng.integers(1, F + 1)):] = 0
    return reads, refs


def _brute(read, ref, sc, affine, w):
    """the per-cell band |i - j| <= w in plain Python: dictionaries of present cells, absent ones simply missing"""
    R, F = len(read), len(ref)
    cls = {ord(c): k for k, c in enumerate("ACGT")}
    cls.update({ord(c.lower()): k for k, c in enumerate("ACGT")})
    if affine:
        o_r, e_r, o_f, e_f = sc.open_read, sc.ext_read, sc.open_ref, sc.ext_ref
    else:
        o_r = e_r = sc.gap_read
        o_f = e_f = sc.gap_ref
    H, E, G = {(-1, -1): 0}, {}, {}
    for j in range(F):
        if abs(-1 - j) <= w:
            H[(-1, j)] = o_r + j * e_r
    for i in range(R):
        if abs(i + 1) <= w:
            H[(i, -1)] = o_f + i * e_f
    for i in range(R):
        for j in range(F):
            if abs(i - j) > w:
                continue
            a, b = cls.get(int(read[i])), cls.get(int(ref[j]))
            s = 0 if a is None or b is None else (sc.match if a == b else sc.mismatch)
            cands = []
            if (i - 1, j - 1) in H:
                cands.append(H[(i - 1, j - 1)] + s)
            e = [v for v in ((E[(i, j - 1)] + e_r) if (i, j - 1) in E else None, (H[(i, j - 1)] + o_r) if (i, j - 1) in H else None) if v is not None]
            g = [v for v in ((G[(i - 1, j)] + e_f) if (i - 1, j) in G else None, (H[(i - 1, j)] + o_f) if (i - 1, j) in H else None) if v is not None]
            if e:
                E[(i, j)] = max(e)
                cands.append(max(e))
            if g:
                G[(i, j)] = max(g)
                cands.append(max(g))
            H[(i, j)] = max(cands)
    Rp = max([i + 1 for i in range(R) if int(read[i]) in cls], default=0)
    Fp = max([j + 1 for j in range(F) if int(ref[j]) in cls], default=0)
    if Rp == 0:
        return [0, 0, 0, 0, 0]
    best, bi, bj = 0, 0, 0
    for i in range(Rp):
        for j in range(Fp):
            if (i, j) in H and H[(i, j)] > best:
                best, bi, bj = H[(i, j)], i + 1, j + 1
    g, gj = None, 0
    for j in range(-1, Fp):
        if (Rp - 1, j) in H and (g is None or H[(Rp - 1, j)] > g):
            g, gj = H[(Rp - 1, j)], j + 1
    return [best, bi, bj, ebr.UNREACHED if g is None else g, gj]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("R,F", [(1, 1), (5, 9), (12, 20), (11, 4)])
def test_per_cell_band_is_the_brute_force_fill(R, F, form):
    reads, refs = _pairs(6, R, F, seed=R * 31 + F)
    sc = _scoring(form)
    affine = len(FORMS[form]) > 2
    for bw in (0, 1, 2, 3, 6, 9, 50):
        got = ebr.extend(reads, refs, sc, bw, affine=affine, B=1)
        exp = [_brute(reads[p], refs[p], sc, affine, bw // 2) for p in range(len(reads))]
        assert got.tolist() == exp, (R, F, form, bw)


@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("form", list(FORMS))
def test_wide_band_is_unbanded(form, B):
    for R, F in ((7, 19), (33, 20), (40, 70)):
        reads, refs = _pairs(5, R, F, seed=R + F)
        sc = _scoring(form)
        affine = len(FORMS[form]) > 2
        exp = extend_ref.extend(reads, refs, sc, affine=affine)
        for bw in (2 * max(R, F), 2 * max(R, F) + 1, 1000):
            assert np.array_equal(ebr.extend(reads, refs, sc, bw, affine=affine, B=B), exp), (R, F, form, bw)


def test_record_agrees_with_the_row_by_row_record():
    reads, refs = _pairs(8, 21, 30, seed=4)
    sc = _scoring("aff")
    Rp, Fp = extend_ref.trimmed_lengths(reads), extend_ref.trimmed_lengths(refs)
    for bw in (1, 4, 11, 30):
        X, P = ebr.matrices(reads, refs, sc, bw, affine=True)
        got = ebr.extend(reads, refs, sc, bw, affine=True)
        assert got.tolist() == [ebr.record(X[p], P, int(Rp[p]), int(Fp[p])) for p in range(8)], bw


@pytest.mark.parametrize("form", list(FORMS))
def test_per_cell_below_block_below_unbanded(form):
    R, F = 37, 52
    reads, refs = _pairs(10, R, F, seed=9)
    sc = _scoring(form)
    affine = len(FORMS[form]) > 2
    free = extend_ref.extend(reads, refs, sc, affine=affine)
    seen_strict = False
    for bw in (1, 2, 5, 10, 17, 40):
        cell = ebr.extend(reads, refs, sc, bw, affine=affine, B=1)
        block = ebr.extend(reads, refs, sc, bw, affine=affine, B=8)
        for col in (0, 3):          # score and gscore; UNREACHED is INT32_MIN, below every value: minus infinity
            assert (cell[:, col] <= block[:, col]).all() and (block[:, col] <= free[:, col]).all(), (form, bw, col)
        seen_strict = seen_strict or (cell[:, 3] < block[:, 3]).any() or (block[:, 3] < free[:, 3]).any()
    assert seen_strict


def test_unreached_closed_form():
    for B in (1, 8):
        for bw in range(0, 40):
            for Rp in range(0, 34):
                for Fp in range(0, 34):
                    P = ebr.present(max(Rp, 1), max(Fp, 1), bw, B)
                    none = Rp > 0 and not P[Rp, :Fp + 1].any()
                    assert ebr.unreached(Rp, Fp, bw, B) == none, (B, bw, Rp, Fp)
    reads = np.full((1, 20), ord("A"), np.uint8)
    refs = np.zeros((1, 30), np.uint8)
    refs[0, :3] = ord("A")
    assert ebr.extend(reads, refs, _scoring("sym"), 4)[0].tolist()[3:] == [ebr.UNREACHED, 0]
