"""The row-table forms of the tilted int16 Smith-Waterman sweep with symmetric affine gaps (score_kernel<G, K, kAlgSW,
kGapAffineSym>, dp_kernels.hip.h: tilted_step) with their adds and their subtract on the 32-bit word and every diagonal taken
from H - (o - x), no H register kept; tests/test_sym_affine_word_arith.py restates the step on the CPU and says which half of
which operand could carry.  Here the geometries of tests/test_gpu_sym_affine_padding_rows.py -- 16 x 10, 8 x 12, 32 x 8 -- and the
8 x 19 side tile with reads of 129, 150 and 152 bases are forced, half-float cells off, every score is compared EXACTLY with
oracle.cpu_ref.score, and describe() says which form ran (ran_score_sym_affine_scores; on the side tile ran_score_sym_affine_form).

Batches of 32 pairs (two waves of the side tile, four of the others):
  * the carry-hazard pairs in both halves of a register (pairs 2g and 2g + 1 share one): a long perfect match -- the read ends
    with the whole reference, the full score lands in the last row at the last column -- beside a pair of mismatches only, beside
    an empty reference, each both ways round;
  * an all-N reference, an empty one, gapped related pairs;
  * `dirty`: the same with an N planted before the last ACGT base of the matching references -- every wave repairs.
References of K + 1, 37 and 60 bases and the two widths whose step counts leave 0 and K - 1 remainder steps.  Scorings: the
benchmark's, x = 0, o - x = 0, the largest table byte exactly 255, shape x scoring at the last match score sym_affine_tilt_ok
admits (largest operand 0x7BFE: the rule keeps one spare unit), and one that leaves the byte rule (mismatch -3, extend -1), on
which the untouched LDS-profile form runs and stays exact."""
import numpy as np
import pytest

from conftest import debug_switches
from oracle import cpu_ref
from test_gpu_sym_affine_max3 import _args, _device, _gapped_pairs
from test_sym_affine_row_tables_sweep import needs_repair, rule_ok
from versalignlib_amd import hipkernel, host

pytestmark = pytest.mark.gpu

SIDE = (8, 19)
EVEN = ((16, 10), (8, 12), (32, 8))
BENCH = (2, -1, -5, -1)
X_ZERO = (3, 1, -4, 0)
OX_ZERO = (2, -1, -1, -1)
BYTE_255 = (249, -1, -5, -1)
NO_BYTE = (2, -3, -5, -1)
EDGE = {(8, 19): (152, 152, (2, -1, -114, -100)), (16, 10): (160, 165, (1, -1, -102, -94))}      # B + x * top + min(R, F) * match = 0x7BFE
N = 32
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_cache = {}


def _lead(R, G, K):
    return (G * K - R) // K if G * K > R else 0


def _widths(R, G, K):
    """K + 1, 37, 60 and the first widths from K + 1 on whose step counts leave 0 and K - 1 remainder steps"""
    steps = lambda F: F + G - 1 - _lead(R, G, K)
    rem = [next(F for F in range(K + 1, K + 1 + K) if steps(F) % K == r) for r in (0, K - 1)]
    assert all(K + 1 <= F <= 60 for F in rem)
    return sorted(set([K + 1, 37, 60] + rem))


def _batch(R, F, dirty, seed=0):
    """-> (reads, refs, {scoring: oracle scores}), cached and read-only"""
    key = (R, F, dirty, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(1000 * R + F + seed)
    reads, refs = _gapped_pairs(N, R, F, seed=R + F + seed)
    reads, refs = reads.copy(), refs.copy()
    hot = []
    for w in range(0, N, 16):
        def match(i):
            refs[i] = ACGT[rng.integers(0, 4, size=F)]
            reads[i] = ACGT[rng.integers(0, 4, size=R)]
            m = min(R, F)
            reads[i, R - m:] = refs[i, F - m:]
            hot.append(i)

        def mismatches(i):
            reads[i], refs[i] = ord("A"), ord("C")

        def empty(i):
            reads[i], refs[i] = ord("G"), 0

        for i, fill in enumerate((match, mismatches, mismatches, match, match, empty, empty, match, match, match)):
            fill(w + i)
        match(w + 10)
        refs[w + 10] = ord("N")                                       # all N: nothing scores, no ACGT base to repair before
        empty(w + 11)
    if dirty:
        for i in hot:
            if refs[i, 0] != ord("N"):
                refs[i, int(rng.integers(0, F - 1))] = ord("N")      # before the last ACGT base
                assert needs_repair(refs[i])
        assert all(any(needs_repair(refs[i]) for i in range(w, w + 16)) for w in range(0, N, 16))    # every wave of the side tile
    else:
        assert not any(needs_repair(r) for r in refs)
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


def _run(monkeypatch, geometry, R, F, scoring, dirty, scores="row_tables"):
    debug_switches(monkeypatch, no_tilt=None, no_row_tables=None, no_side_tile=None)
    batch = _batch(R, F, dirty)
    reads, refs, _ = batch
    exp = _expected(batch, scoring)
    what = (geometry, R, F, scoring, "dirty" if dirty else "clean")
    if not dirty:                                                     # the hazard: a full score beside a pair that scores nothing
        cold = min(R, F) * max(scoring[1], 0)
        assert exp[0] == exp[3] == min(R, F) * scoring[0] and exp[1] == exp[2] == cold and exp[5] == exp[6] == exp[10] == exp[11] == 0, what
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*_args(scoring)), group_lanes=geometry[0], rows_per_lane=geometry[1])
    eng.set_half_float_cells(0)
    got = eng.score_device(host.SW, _device(reads.copy()), _device(refs.copy())).cpu().numpy()
    d = eng.describe(host.SW, N)
    eng.close()
    bad = np.nonzero(got != exp)[0]
    assert not bad.size, what + (bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist())
    assert d["ran_score_cells"] == "int16" and d["ran_score_geometry"] == "%dx%d" % geometry, what + (d,)
    assert d["ran_score_sym_affine"] == "max3" and d["ran_score_sym_affine_frame"] == "tilted", what + (d,)
    assert d["ran_score_sym_affine_scores"] == scores, what + (d["ran_score_sym_affine_scores"],)
    if geometry == SIDE:
        assert d["ran_score_sym_affine_form"] == ("row_tables_repair" if dirty else "row_tables"), what + (d["ran_score_sym_affine_form"],)


@pytest.mark.parametrize("dirty", (False, True), ids=("clean", "dirty"))
@pytest.mark.parametrize("R", (129, 150, 152))
def test_the_side_tile(monkeypatch, R, dirty):
    for F in _widths(R, *SIDE):
        _run(monkeypatch, SIDE, R, F, BENCH, dirty)


@pytest.mark.parametrize("dirty", (False, True), ids=("clean", "dirty"))
@pytest.mark.parametrize("geometry", EVEN, ids=lambda g: "%dx%d" % g)
def test_the_even_tiles(monkeypatch, geometry, dirty):
    G, K = geometry
    for R in (G * K - K, G * K):                                      # a padding lane, none
        for F in _widths(R, G, K):
            _run(monkeypatch, geometry, R, F, BENCH, dirty)


@pytest.mark.parametrize("scoring", (X_ZERO, OX_ZERO, BYTE_255), ids=("x0", "ox0", "byte255"))
def test_scorings_at_the_operands_edges(monkeypatch, scoring):
    assert rule_ok(*scoring)
    for geometry, R in ((SIDE, 150), (SIDE, 152), ((16, 10), 150), ((8, 12), 96), ((32, 8), 250)):
        for dirty in (False, True):
            _run(monkeypatch, geometry, R, 37, scoring, dirty)


@pytest.mark.parametrize("geometry", sorted(EDGE), ids=lambda g: "%dx%d" % g)
def test_the_last_scoring_the_tilted_window_admits(monkeypatch, geometry):
    R, F, scoring = EDGE[geometry]
    o, x = -scoring[2], -scoring[3]
    lead = _lead(R, *geometry)
    assert 1024 + max(o - x, -scoring[1]) + x * (geometry[0] * geometry[1] + F - lead) + min(R, F) * scoring[0] == 0x7BFE
    for dirty in (False, True):
        _run(monkeypatch, geometry, R, F, scoring, dirty)


@pytest.mark.parametrize("geometry", EVEN, ids=lambda g: "%dx%d" % g)
def test_a_score_that_is_no_byte_keeps_the_lds_profile(monkeypatch, geometry):
    """mismatch' = -1: the form whose packed instructions stay; same batches, same exactness"""
    assert not rule_ok(*NO_BYTE)
    G, K = geometry
    for F in (K + 1, 37):
        for dirty in (False, True):
            _run(monkeypatch, geometry, G * K - K, F, NO_BYTE, dirty, scores="lds_profile")
