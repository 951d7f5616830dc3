"""The int16 Smith-Waterman sweep with symmetric affine gaps (score_kernel<G, K, kAlgSW, kGapAffineSym>, dp_kernels.hip.h):
it carries the best SOURCE of a gap per cell instead of the gap's score and feeds the running maximum once per pair of
steps, with max(XE, XF) of the second step plus its last row (tests/test_sym_affine_gap_sources.py restates the sweep on
the CPU).  Everything here runs on int16 cells (set_half_float_cells(0)) and is compared EXACTLY with oracle.cpu_ref.score:
one-hot batches in which a single cell can supply the score -- at every (row, column), so also the last row of a lane on a
first and on a second step, the last lane, the last column, the leftover step of an odd count and the lanes above the
sweep's first lane --, random related pairs at the short shapes where fill and drain overlap, on the engine's geometry and
on 32-lane groups (whose hand-over of XF is a wave shift, not a DPP row shift), and reads with long deletions and
insertions at the bench shape.  The NW variant, whose kernel keeps gap scores, runs through the same cases as the control.

One scoring of the list, (open, extend) = (-2, -3), is no affine model (an extension dearer than the opening) and the engine
refuses it at construction (Engine::validate_scoring): the cases keep it and check exactly that; the recurrence itself is
checked with it on the CPU."""
import numpy as np
import pytest

from oracle import cpu_ref
from versalignlib_amd import hipkernel, host

pytestmark = pytest.mark.gpu

GAPS = ((-5, -1), (-1, -1), (-2, -3), (-4, 0), (0, 0))          # (open, extend), the same for both directions
SUBS = ((2, -1), (5, -4))
SCORINGS = [sub + gaps for gaps in GAPS for sub in SUBS]
ALGS = (host.SW, host.NW)

_oracle_cache = {}


def _args(scoring):
    match, mismatch, gap_open, gap_ext = scoring
    return (match, mismatch, -3, -3, gap_open, gap_ext, gap_open, gap_ext)


def _oracle(key, alg, scoring, reads, refs):
    """cpu_ref.score of a case, computed once and shared by every geometry and batch size (read-only)."""
    k = (key, alg, scoring)
    if k not in _oracle_cache:
        exp = cpu_ref.score(alg, reads, refs, cpu_ref.Scoring.make(*_args(scoring)), threads=4, affine=True)
        exp.setflags(write=False)
        _oracle_cache[k] = exp
    return _oracle_cache[k]


def _refused(scoring):
    """(open, extend) with extend < open: the engine refuses it, and that is what its cases check."""
    if scoring[3] >= scoring[2]:
        return False
    with pytest.raises(hipkernel.HipKernelError, match="extend >= open"):
        hipkernel.Engine(150, 500, hipkernel.Scoring.make(*_args(scoring)))
    return True


def _engine(R, F, scoring, geometry=None):
    G, K = geometry or (0, 0)
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*_args(scoring)), group_lanes=G, rows_per_lane=K)
    eng.set_half_float_cells(0)
    return eng


def _check(eng, alg, d_reads, d_refs, exp, geometry, what):
    n = int(d_reads.shape[0])
    got = eng.score_device(alg, d_reads, d_refs).cpu().numpy()
    bad = np.nonzero(got != exp[:n])[0]
    assert not bad.size, what + (alg, bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist())
    d = eng.describe(alg, n)
    assert d["ran_score_cells"] == "int16", what + (d,)
    if geometry:
        assert d["ran_score_geometry"] == "%dx%d" % geometry, what + (d,)


def _device(a):
    import torch
    return torch.from_numpy(a).cuda()


# ---- 1. one matching base at (row i, column j), everything else mismatches: only that cell can supply the score ----
def _one_hot(R, F):
    n = R * F
    reads, refs = np.full((n, R), ord("A"), dtype=np.uint8), np.full((n, F), ord("C"), dtype=np.uint8)
    i, j = np.divmod(np.arange(n), F)
    reads[np.arange(n), i] = ord("G")
    refs[np.arange(n), j] = ord("G")
    return reads, refs


@pytest.mark.parametrize("scoring", SCORINGS)
def test_one_matching_base_at_every_cell(scoring):
    if _refused(scoring):
        return
    for R in (160, 150, 11):
        for F in (5, 6):                                   # both parities of the step count
            reads, refs = _one_hot(R, F)
            d_reads, d_refs = _device(reads), _device(refs)
            for geometry in (None, (16, 10)):
                eng = _engine(R, F, scoring, geometry)
                for alg in ALGS:
                    exp = _oracle(("one_hot", R, F), alg, scoring, reads, refs)
                    if alg == host.SW:
                        assert (exp == scoring[0]).all()          # the match score, from the one cell that has it
                    _check(eng, alg, d_reads, d_refs, exp, geometry, ("one_hot", R, F, geometry))
                eng.close()


# ---- 2. random related pairs where fill and drain overlap, the step count changes parity, tail waves ----
EDGE_F = (1, 2, 15, 16, 17, 31, 32)
EDGE_R = (1, 9, 10, 11, 150, 160)
EDGE_N = (1, 7, 9, 64)


def _related_pairs(n, R, F, seed):
    """ACGT references; every read is random ACGT with a mutated piece of its reference copied in."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    refs = acgt[rng.integers(0, 4, size=(n, F))]
    reads = acgt[rng.integers(0, 4, size=(n, R))]
    piece = min(R, F)
    for i in range(n):
        m = int(rng.integers(1, piece + 1))
        a, b = int(rng.integers(0, F - m + 1)), int(rng.integers(0, R - m + 1))
        reads[i, b:b + m] = refs[i, a:a + m]
    flip = rng.random((n, R)) < 0.1
    reads[flip] = acgt[rng.integers(0, 4, size=int(flip.sum()))]
    return np.ascontiguousarray(reads), np.ascontiguousarray(refs)


@pytest.mark.parametrize("geometry", [None, (32, 10)], ids=["own", "32x10"])
@pytest.mark.parametrize("scoring", SCORINGS)
def test_short_sweeps_every_parity_and_tail(scoring, geometry):
    if _refused(scoring):
        return
    for R in EDGE_R:
        for F in EDGE_F:
            reads, refs = _related_pairs(max(EDGE_N), R, F, seed=1000 * R + F)
            d_reads, d_refs = _device(reads), _device(refs)
            eng = _engine(R, F, scoring, geometry)
            for alg in ALGS:
                exp = _oracle(("edge", R, F), alg, scoring, reads, refs)
                for n in EDGE_N:
                    _check(eng, alg, d_reads[:n], d_refs[:n], exp, geometry, ("edge", R, F, n, geometry))
            eng.close()


# ---- 3. reads with pieces of 1 to 12 bases deleted or inserted against their reference: long gaps in both directions ----
def _gapped_pairs(n, R, F, seed):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    refs = acgt[rng.integers(0, 4, size=(n, F))]
    reads = np.empty((n, R), dtype=np.uint8)
    for i in range(n):
        out, pos = [], int(rng.integers(0, F - R - 60))
        while sum(len(p) for p in out) < R:
            run = int(rng.integers(8, 30))
            out.append(refs[i, pos:pos + run])
            pos += run
            gap = int(rng.integers(1, 13))
            if rng.random() < 0.5:
                pos += gap                                              # deleted from the read
            else:
                out.append(acgt[rng.integers(0, 4, size=gap)])          # inserted into the read
        reads[i] = np.concatenate(out)[:R]
    return np.ascontiguousarray(reads), np.ascontiguousarray(refs)


@pytest.mark.parametrize("scoring", SCORINGS)
def test_long_gaps_in_both_directions(scoring):
    if _refused(scoring):
        return
    R, F, n = 150, 500, 64
    reads, refs = _gapped_pairs(n, R, F, seed=150500)
    d_reads, d_refs = _device(reads), _device(refs)
    eng = _engine(R, F, scoring)
    for alg in ALGS:
        exp = _oracle(("gapped", R, F), alg, scoring, reads, refs)
        if alg == host.SW and scoring[2:] == (-5, -1):
            # the gaps are used: no ungapped piece of a read (at most 29 bases) reaches these scores
            assert (exp > 29 * scoring[0]).all()
        _check(eng, alg, d_reads, d_refs, exp, None, ("gapped", R, F))
    eng.close()
