"""tests/extend_ref.py -- the numpy restatement the GPU tests of the extension scores compare against -- pinned on the CPU to
the exhaustive enumerator (tests/enumerate_alignments.py: every DIAG / UP / LEFT path from the origin, maximal gap runs priced
open + (k - 1) * ext), cell by cell and record by record, on every shape from 1 x 1 to 5 x 6; then its invariants on planted
40 x 60 pairs, and the rule's bound (extend_choice, asked through tests/extend_rules_check.cpp) held against the restatement's own
smallest and largest cells on adversarial pairs."""
import os
import subprocess

import numpy as np
import pytest

import enumerate_alignments as enum
import extend_ref
from conftest import ROOT
from oracle import cpu_ref
from versalignlib_amd import hipkernel

BASES = np.frombuffer(b"ACGT", np.uint8)
# (match, mismatch, open_read, ext_read, open_ref, ext_ref): asymmetric affine with open != extend, symmetric affine, and
# linear scorings stated as open = ext
AFFINE = [(2, -1, -5, -1, -4, -2), (3, -2, -4, -1, -4, -1), (1, -3, -2, -2, -6, -1)]
LINEAR = [(2, -1, -3, -3, -3, -3), (2, -1, -2, -2, -4, -4)]


def _scoring(sc, affine):
    m, x, o_r, e_r, o_f, e_f = sc
    return hipkernel.Scoring.make(m, x, o_r, o_f, o_r, e_r, o_f, e_f) if affine else hipkernel.Scoring.make(m, x, o_r, o_f)


def _random_pair(rng, R, F):
    """random bases, a tail of N or NUL on some, interior junk bytes (N, NUL, a byte >= 0x80, lower case) on some"""
    read, ref = BASES[rng.integers(0, 4, R)].copy(), BASES[rng.integers(0, 4, F)].copy()
    if rng.random() < 0.5:
        k = min(R, F)
        ref[:k] = read[:k]                      # an extension that scores
    for s in (read, ref):
        if rng.random() < 0.4:
            s[rng.integers(0, len(s) + 1):] = rng.choice([0, ord("N")])
        if rng.random() < 0.4:
            s[rng.integers(0, len(s))] = rng.choice([0, ord("N"), 0x80, 0xC1, ord("n")])
        if rng.random() < 0.3:
            s[rng.integers(0, len(s))] |= 0x20          # lower case is the same base
    return read, ref


@pytest.mark.parametrize("R", range(1, 6))
def test_cells_and_records_equal_the_enumerator(R):
    rng = np.random.default_rng(R)
    for F in range(1, 7):
        for k, (sc, affine) in enumerate([(s, True) for s in AFFINE] + [(s, False) for s in LINEAR]):
            read, ref = _random_pair(rng, R, F)
            X = extend_ref.matrices(read[None, :], ref[None, :], _scoring(sc, affine), affine)[0]
            cells = enum.best_ending_at(bytes(read), bytes(ref), sc, [(0, 0)])
            assert len(cells) == (R + 1) * (F + 1)
            for (i, j), v in cells.items():
                assert X[i, j] == v, (R, F, sc, bytes(read), bytes(ref), i, j, int(X[i, j]), v)
            # the record, derived from the enumerated cells
            Rp, Fp = int(extend_ref.trimmed_lengths(read[None, :])[0]), int(extend_ref.trimmed_lengths(ref[None, :])[0])
            table = np.array([[cells[(i, j)] for j in range(F + 1)] for i in range(R + 1)], np.int64)
            got = extend_ref.extend(read[None, :], ref[None, :], _scoring(sc, affine), affine)[0].tolist()
            assert got == extend_ref.record(table, Rp, Fp), (R, F, sc, bytes(read), bytes(ref))
            if Rp == 0:
                assert got == [0, 0, 0, 0, 0]
            if got[0] == 0:
                assert got[:3] == [0, 0, 0]


def test_borders_by_hand():
    sc = hipkernel.Scoring.make(2, -1, -3, -3, -5, -1, -4, -2)
    X = extend_ref.matrices(np.frombuffer(b"ACG", np.uint8)[None, :], np.frombuffer(b"ACGT", np.uint8)[None, :], sc, True)[0]
    assert X[0].tolist() == [0, -5, -6, -7, -8] and X[:, 0].tolist() == [0, -4, -6, -8]
    assert [int(X[k, k]) for k in range(4)] == [0, 2, 4, 6]
    lin = hipkernel.Scoring.make(2, -1, -3, -2)
    X = extend_ref.matrices(np.frombuffer(b"ACG", np.uint8)[None, :], np.frombuffer(b"ACGT", np.uint8)[None, :], lin, False)[0]
    assert X[0].tolist() == [0, -3, -6, -9, -12] and X[:, 0].tolist() == [0, -2, -4, -6]
    # the first bases all mismatch: no cell above 0, the read-end score is negative and may sit in the border column
    got = extend_ref.extend(np.frombuffer(b"AAA", np.uint8)[None, :], np.frombuffer(b"CCCC", np.uint8)[None, :], lin)
    assert got.tolist() == [[0, 0, 0, -3, 3]]
    got = extend_ref.extend(np.frombuffer(b"AAA", np.uint8)[None, :], np.frombuffer(b"CCCC", np.uint8)[None, :], hipkernel.Scoring.make(2, -9, -3, -1))
    assert got.tolist() == [[0, 0, 0, -3, 0]]
    # a read longer than the trimmed reference does not ride its tail down the padding: columns at or beyond Fp are no candidates
    rd, rf = np.frombuffer(b"ACGTACGT", np.uint8), np.frombuffer(b"ACGT\0\0\0\0\0\0", np.uint8)
    assert extend_ref.extend(rd[None, :], rf[None, :], lin).tolist() == [[8, 4, 4, 0, 4]]
    assert int(extend_ref.matrices(rd[None, :], rf[None, :], lin)[0][8, 8]) == 8          # ... which an untrimmed row maximum would report


def _planted(n, R, F, seed):
    rng = np.random.default_rng(seed)
    reads, refs = BASES[rng.integers(0, 4, (n, R))], BASES[rng.integers(0, 4, (n, F))]
    for p in range(n):
        L = R if p % 4 == 3 else int(rng.integers(1, R + 1))           # (a quarter: the whole read is the reference's prefix)
        refs[p, :L] = reads[p, :L]                                       # an extension from the anchor ...
        if p % 3 == 0 and L > 8:
            refs[p, L // 2] = BASES[(int(np.searchsorted(BASES, refs[p, L // 2])) + 1) % 4]      # ... with a mismatch
        if p % 4 == 1:
            reads[p, int(rng.integers(R // 2, R)):] = rng.choice([0, ord("N")])
        if p % 4 == 2:
            refs[p, int(rng.integers(F // 2, F)):] = rng.choice([0, ord("N")])
    return reads, refs


@pytest.mark.parametrize("affine", [False, True])
def test_invariants_on_planted_pairs(affine):
    reads, refs = _planted(64, 40, 60, seed=5)
    sc = hipkernel.Scoring.make(2, -1, -3, -3, -5, -1, -5, -1) if affine else hipkernel.Scoring.make(2, -1, -3, -3)
    got = extend_ref.extend(reads, refs, sc, affine)
    oracle_sc = cpu_ref.Scoring.make(2, -1, -3, -3, -5, -1, -5, -1) if affine else cpu_ref.Scoring.make(2, -1, -3, -3)
    sw = np.asarray(cpu_ref.score(0, reads, refs, oracle_sc, affine=affine), np.int64)          # the oracle's Smith-Waterman score
    assert (got[:, 0] <= sw).all()
    Fp = extend_ref.trimmed_lengths(refs)
    assert (got[Fp > 0, 3] <= got[Fp > 0, 0]).all()
    assert (got[:, 0] > 0).any() and (got[:, 3] < got[:, 0]).any()
    # the read equals the reference prefix
    Rp = extend_ref.trimmed_lengths(reads)
    same = np.array([np.array_equal(reads[p, :Rp[p]], refs[p, :Rp[p]]) for p in range(len(reads))]) & (Rp > 0)
    assert same.sum() >= 8
    for p in np.nonzero(same)[0]:
        assert got[p].tolist() == [2 * Rp[p], Rp[p], Rp[p], 2 * Rp[p], Rp[p]], (p, got[p].tolist())


# ---- the rule's bound against the restatement's own cells ----
def _rule(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("extend_rule") / "extend_rules_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "versalignlib_amd", "csrc"),
                            os.path.join(ROOT, "tests", "extend_rules_check.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]

    def ask(R, F, m, x, affine, o_r, e_r, o_f, e_f):
        res = subprocess.run([exe] + [str(v) for v in (R, F, m, x, o_r, o_f, int(affine), o_r, e_r, o_f, e_f)], stdout=subprocess.PIPE, text=True, timeout=60)
        word, top, bottom = res.stdout.split()
        return word == "accept", int(top), int(bottom)
    return ask


def test_accepted_shapes_keep_adversarial_cells_inside_int16(tmp_path_factory):
    ask = _rule(tmp_path_factory)
    accepted = 0
    for R, F in ((40, 60), (60, 40), (33, 33), (150, 70)):
        for affine, (m, x, o_r, e_r, o_f, e_f) in [(False, (2, -1, -3, -3, -3, -3)), (False, (500, -400, -300, -300, -200, -200)), (False, (800, -700, -10, -10, -500, -500)),
                                                   (False, (3, 700, -3, -3, -3, -3)), (True, (2, -1, -5, -1, -4, -2)), (True, (600, -500, -400, -1, -300, -2)),
                                                   (True, (100, -900, -250, -250, -150, -100)), (False, (900, -1, -1, -1, -1, -1)), (True, (2, -1, -330, -1, -1, -1))]:
            ok, top, bottom = ask(R, F, m, x, affine, o_r, e_r, o_f, e_f)
            if not ok:
                continue
            accepted += 1
            sc = hipkernel.Scoring.make(m, x, o_r, o_f, o_r, e_r, o_f, e_f) if affine else hipkernel.Scoring.make(m, x, o_r, o_f)
            a_read, a_ref = np.full(R, ord("A"), np.uint8), np.full(F, ord("A"), np.uint8)
            c_ref, empty = np.full(F, ord("C"), np.uint8), np.zeros(F, np.uint8)
            reads = np.stack([a_read, a_read, a_read])
            refs = np.stack([c_ref, a_ref, empty])              # all-mismatch, all-match, a read against an empty reference
            X = extend_ref.matrices(reads, refs, sc, affine)
            assert X.max() <= top <= 32000 and X.min() >= bottom >= -32000, (R, F, m, x, affine, int(X.max()), top, int(X.min()), bottom)
            assert X.max() <= 32767 and X.min() >= -32768
    assert accepted >= 12
