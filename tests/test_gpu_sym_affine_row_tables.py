"""The tilted int16 Smith-Waterman sweep with symmetric affine gaps (score_kernel<G, K, kAlgSW, kGapAffineSym>,
dp_kernels.hip.h) takes its substitution scores from ROW TABLES in registers where every one of them is a byte
(cell_rules.h: sym_affine_row_tables_ok; tests/test_sym_affine_row_tables_sweep.py restates the step on the CPU), and from
the LDS profile everywhere else and under VALIGN_HIP_DEBUG=no_row_tables.  Everything here runs on int16 cells, is compared
EXACTLY with oracle.cpu_ref.score and asserts through describe() which of the two ran (ran_score_sym_affine_scores):

  a. on 16x10, 8x12, 16x8 and 32x8, reads of G K - K - 1, G K - K, G K - 1 and G K bases (one lane of padding rows and a row, that
     lane exactly, one padding row, none) against references of 1, G - 1, G, G + 1 and 64 bases.  Every batch mixes, in blocks of 16
     pairs (a whole number of waves on every geometry): clean pairs; ONE pair with an N inside its reference; N runs in reads;
     NUL-padded short reads and references; a base that is no ACGT at column 0 of the reference; one at the column before the
     last ACGT base; all of that at random -- so waves of the plain row-table step and of its repairing copy both run;
  b. a reference of 261 bases (two trips of the stream's set-up, a rim of one column) and a last wave that is not full;
  c. a scoring the rule refuses (mismatch' = -1): the LDS profile, the same scores;
  d. the debug switch on a scoring the rule accepts."""
import numpy as np
import pytest

from conftest import debug_switches
from oracle import cpu_ref
from test_gpu_sym_affine_max3 import _args, _device
from versalignlib_amd import hipkernel, host

pytestmark = pytest.mark.gpu

GEOMETRIES = ((16, 10), (8, 12), (16, 8), (32, 8))
ACCEPTED = (2, -1, -5, -1)          # x = 1, o - x = 4: match' 4, mismatch' 1, zero' 2, row 0 at most 8
REFUSED = (2, -3, -5, -1)           # mismatch' = -3 + 2 = -1

_cache = {}


def _batch(R, F, blocks=7, seed=0):
    """blocks x 16 pairs: a read with a mutated copy of (a piece of) its reference somewhere in it, then block by block the
    bases that score nothing.  Cached with its oracle scores per scoring (read-only)."""
    key = (R, F, blocks, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(1000003 * R + 1009 * F + seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    n = 16 * blocks
    refs = np.ascontiguousarray(acgt[rng.integers(0, 4, size=(n, F))])
    reads = np.ascontiguousarray(acgt[rng.integers(0, 4, size=(n, R))])
    for i in range(n):
        piece = refs[i, int(rng.integers(0, max(1, F // 3))):][:R].copy()
        if piece.size > 6:                                            # a deletion, a substitution
            cut = int(rng.integers(1, piece.size - 4))
            piece = np.concatenate((piece[:cut], piece[cut + int(rng.integers(1, 4)):]))
            piece[int(rng.integers(0, piece.size))] = acgt[int(rng.integers(0, 4))]
        at = int(rng.integers(0, R - piece.size + 1))
        reads[i, at:at + piece.size] = piece

    def short(i):                                                     # the reference's ACGT columns end somewhere inside
        keep = int(rng.integers(1, F + 1))
        refs[i, keep:] = 0
        return keep

    for i in range(n):
        block, k = divmod(i, 16)
        kinds = (block,) if block < 6 else tuple(int(v) for v in rng.integers(1, 6, size=2))
        for kind in kinds:
            if kind == 1 and (block != 1 or k == 3):                  # block 1: one pair of the wave only
                refs[i, int(rng.integers(0, F))] = ord("N")
            elif kind == 2:
                a = int(rng.integers(0, R - 1))
                reads[i, a:a + int(rng.integers(1, 13))] = ord("N")
            elif kind == 3:
                short(i)
                reads[i, int(rng.integers(1, R)):] = 0
            elif kind == 4:
                refs[i, 0] = ord("N") if k % 2 else ord("x")
            elif kind == 5:
                keep = short(i) if k % 2 else F
                if keep >= 2:
                    refs[i, keep - 2] = ord("N")
    reads.setflags(write=False)
    refs.setflags(write=False)
    _cache[key] = (reads, refs, {})
    return _cache[key]


def _expected(batch, scoring):
    reads, refs, oracle = batch
    if scoring not in oracle:
        exp = cpu_ref.score(host.SW, reads, refs, cpu_ref.Scoring.make(*_args(scoring)), threads=4, affine=True)
        exp.setflags(write=False)
        oracle[scoring] = exp
    return oracle[scoring]


def _run(monkeypatch, R, F, geometry, scoring, scores, batch, n=None, switch=False):
    debug_switches(monkeypatch, no_row_tables=1 if switch else None)
    reads, refs, _ = batch
    exp = _expected(batch, scoring)
    n = n or reads.shape[0]
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*_args(scoring)), group_lanes=geometry[0], rows_per_lane=geometry[1])
    eng.set_half_float_cells(0)
    got = eng.score_device(host.SW, _device(reads[:n].copy()), _device(refs[:n].copy())).cpu().numpy()
    d = eng.describe(host.SW, n)
    eng.close()
    what = (R, F, geometry, scoring, scores)
    bad = np.nonzero(got != exp[:n])[0]
    assert not bad.size, what + (bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist())
    assert d["ran_score_cells"] == "int16" and d["ran_score_geometry"] == "%dx%d" % geometry, what + (d,)
    assert d["ran_score_sym_affine"] == "max3" and d["ran_score_sym_affine_frame"] == "tilted", what + (d,)
    assert d["ran_score_sym_affine_scores"] == scores, what + (d["ran_score_sym_affine_scores"],)


def _read_lengths(G, K):
    return (G * K - K - 1, G * K - K, G * K - 1, G * K)


# ---- a. the shapes around a lane of padding rows and around the lane group's width, every kind of base that scores nothing ----
@pytest.mark.parametrize("which", range(4), ids=("GK-K-1", "GK-K", "GK-1", "GK"))
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_row_tables_against_the_oracle(monkeypatch, geometry, which):
    G, K = geometry
    R = _read_lengths(G, K)[which]
    for F in (1, G - 1, G, G + 1, 64):
        batch = _batch(R, F)
        assert _expected(batch, ACCEPTED).max() > 0 or F == 1
        _run(monkeypatch, R, F, geometry, ACCEPTED, "row_tables", batch)


# ---- b. two trips and a rim in the stream's set-up; a last wave with one pair ----
def test_long_reference_and_short_last_wave(monkeypatch):
    _run(monkeypatch, 150, 261, (16, 10), ACCEPTED, "row_tables", _batch(150, 261, blocks=8, seed=5), n=16 * 7 + 1)
    _run(monkeypatch, 96, 261, (8, 12), ACCEPTED, "row_tables", _batch(96, 261, blocks=8, seed=5), n=16 * 7 + 3)


# ---- c. mismatch' = -1 is no byte: the LDS profile runs, in the tilted frame, with the same scores ----
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_refused_scoring_runs_the_lds_profile(monkeypatch, geometry):
    G, K = geometry
    R = G * K - 1
    _run(monkeypatch, R, 64, geometry, REFUSED, "lds_profile", _batch(R, 64))


# ---- d. the debug switch ----
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_debug_switch_forces_the_lds_profile(monkeypatch, geometry):
    G, K = geometry
    R = G * K - 1
    _run(monkeypatch, R, 64, geometry, ACCEPTED, "lds_profile", _batch(R, 64), switch=True)
    _run(monkeypatch, R, 64, geometry, ACCEPTED, "row_tables", _batch(R, 64))
