"""tests/placed_ref.py -- the numpy restatement the GPU tests of the placed scores compare against -- pinned on the CPU: its
scores are the oracle's, its ends the plain-Python end cells of tests/cigar_ref.py, and on every Smith-Waterman fixture under
tests/golden the stored alignment lies where it says the alignment ends."""
import glob
import os

import numpy as np
import pytest

import cigar_ref
import placed_ref
from conftest import ROOT
from oracle import cpu_ref
from versalignlib_amd import synth

LINEAR = [cpu_ref.Scoring.make(), cpu_ref.Scoring.make(3, -2, -4, -2), cpu_ref.Scoring.make(1, -3, -1, -5)]
AFFINE = [cpu_ref.Scoring.make(2, -1, -3, -3, -5, -1, -5, -1), cpu_ref.Scoring.make(2, -1, -3, -3, -6, -2, -4, -1),
          cpu_ref.Scoring.make(3, -2, -3, -3, -2, -2, -7, 0)]


def _pairs(n, R, F, seed):
    reads, refs = synth.make_pairs(n, R, F, seed=seed, indel_rate=0.03)
    rng = np.random.default_rng(seed)
    reads[rng.random(reads.shape) < 0.02] = ord("N")
    refs[rng.random(refs.shape) < 0.02] = ord("n")
    return reads, refs


@pytest.mark.parametrize("affine", [False, True])
def test_scores_are_the_oracles(affine):
    for k, sc in enumerate(AFFINE if affine else LINEAR):
        for R, F in ((33, 70), (150, 210), (64, 17)):
            reads, refs = _pairs(48, R, F, 100 * k + R)
            got = placed_ref.placed(reads, refs, sc, affine=affine)
            assert np.array_equal(got[:, 0], cpu_ref.score(0, reads, refs, sc, affine=affine).astype(np.int64)), (k, R, F)


@pytest.mark.parametrize("affine", [False, True])
def test_ends_are_the_plain_python_end_cells(affine):
    for k, sc in enumerate(AFFINE if affine else LINEAR):
        for R, F in ((40, 60), (12, 20), (31, 9)):
            reads, refs = _pairs(32, R, F, 7 * k + F)
            # low-complexity pairs: many cells share the maximum
            reads[:8] = np.frombuffer(b"ACAC" * R, np.uint8)[:R]
            refs[:8] = np.frombuffer(b"ACAC" * F, np.uint8)[:F]
            got = placed_ref.placed(reads, refs, sc, affine=affine)
            ends = cigar_ref.end_cells_sw(reads, refs, sc, affine=affine)
            exp = np.where(got[:, :1] > 0, ends + 1, 0)
            assert np.array_equal(got[:, 1:], exp), (k, R, F, got[:4], exp[:4])


def _fixture_cases():
    cases = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz"))):
        cases.append((path, None))
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "affine", "*.npz"))):
        cases.append((path, "affine"))
    return cases


@pytest.mark.parametrize("path,kind", _fixture_cases(), ids=lambda v: os.path.basename(v) if isinstance(v, str) and v.endswith(".npz") else str(v))
def test_golden_alignments_lie_where_the_ends_say(path, kind):
    g = np.load(path)
    reads, refs = g["reads"], g["refs"]
    if kind is None:
        m, x, gr, gf = (int(v) for v in g["scoring"])
        sets = [(cpu_ref.Scoring.make(m, x, gr, gf), False, g["rows_sw"], g["idx_sw"], g["score_sw"])]
    else:
        sets = []
        for s, sc in enumerate(g["scorings"].tolist()):
            osc = cpu_ref.Scoring.make(sc[0], sc[1], sc[2], sc[4], sc[2], sc[3], sc[4], sc[5])
            sets.append((osc, True, g["rows_sw_%d" % s], g["idx_sw_%d" % s], g["sw_score_%d" % s]))
    for sc, affine, rows, idx, score in sets:
        got = placed_ref.placed(reads, refs, sc, affine=affine)
        assert np.array_equal(got[:, 0], score.astype(np.int64)), path
        for p, (a, b) in enumerate(cigar_ref.degapped(rows, idx)):
            re_, fe = int(got[p, 1]), int(got[p, 2])
            if got[p, 0] == 0:
                assert (re_, fe) == (0, 0) and not a and not b, (path, p)
                continue
            assert reads[p, re_ - len(a):re_].tobytes() == a and re_ - len(a) >= 0, (path, p, "read", re_)
            assert refs[p, fe - len(b):fe].tobytes() == b and fe - len(b) >= 0, (path, p, "ref", fe)


def test_all_n_reads_are_empty():
    reads, refs = _pairs(16, 30, 50, 5)
    reads[:] = ord("N")
    for sc, affine in ((LINEAR[0], False), (AFFINE[0], True)):
        assert not placed_ref.placed(reads, refs, sc, affine=affine).any()


def test_long_shape_runs_in_seconds():
    reads, refs = synth.make_pairs(2, 1100, 1300, seed=3, indel_rate=0.02)
    got = placed_ref.placed(reads, refs, AFFINE[0], affine=True)
    assert np.array_equal(got[:, 0], cpu_ref.score(0, reads, refs, AFFINE[0], affine=True).astype(np.int64))
