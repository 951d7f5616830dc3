"""The tilted frame of the biased int16 Smith-Waterman sweep with symmetric affine gaps (score_kernel<G, K, kAlgSW,
kGapAffineSym>, dp_kernels.hip.h) as it runs now: running maxima carried inside the frame and taken out once, `ho` handed
across the lane boundary with o - x in the profile scores of a lane's row 0 (zero slab included), remainder steps as the tail
of a trip.  tests/test_sym_affine_inframe_sweep.py restates it on the CPU; here every geometry of at most 12 rows per lane is
forced as tests/test_gpu_sym_affine_tilted.py forces it, on int16 cells, and compared EXACTLY with oracle.cpu_ref.score:

  a. reads that leave 1, 0 and 1 padding lanes (16x10: 150, 160 and 141 bases) against references of 1, 9, 10, 11 and 37
     bases and of widths whose step counts leave 0, 1 and K - 1 remainder steps; each batch holds gapped related pairs, a read
     of bases that score nothing, one matching base on the first and on the last anti-diagonal, and two matching bases in a
     row of which the second lies in a lane's row 0 (its score arrives by the diagonal from the lane above);
  b. the same batch under VALIGN_HIP_DEBUG=no_tilt: the plain frame, whose profile must not carry the addend;
  c. an NW score on the same engine after a tilted launch: the other users of the set-up do not get it either;
  d. references too long to be staged with the reads: the set-up's other way of building the profile."""
import numpy as np
import pytest

import instance_matrix as im
from conftest import debug_switches
from oracle import cpu_ref
from test_gpu_sym_affine_max3 import _args, _device, _gapped_pairs
from versalignlib_amd import hipkernel, host

pytestmark = pytest.mark.gpu

GEOMS = sorted(g for g in im.GEOMETRIES if g[1] <= 12)
SCORING = (2, -1, -5, -1)
N = 256


def _lead(R, G, K):
    return (G * K - R) // K if G * K > R else 0


def _steps(R, F, G, K):
    return F + G - 1 - _lead(R, G, K)


def _remainder_widths(R, G, K):
    """The smallest reference widths whose step counts leave 0, 1 and K - 1 remainder steps."""
    return [next(F for F in range(1, K + 1) if _steps(R, F, G, K) % K == r) for r in (0, 1, K - 1)]


def _batch(R, F, G, K, seed):
    reads, refs = _gapped_pairs(N, R, F, seed)
    top = G * K - R                                                   # padding rows above the read
    reads[0] = np.frombuffer(b"NnXN" * R, dtype=np.uint8)[:R]         # scores nothing anywhere
    for i, (r, c) in ((1, (0, 0)), (2, (R - 1, F - 1))):              # the first and the last anti-diagonal
        reads[i], refs[i] = ord("A"), ord("C")
        reads[i, r], refs[i, c] = ord("G"), ord("G")
    row0 = [r for r in range(1, R) if (top + r) % K == 0]             # read positions in a lane's row 0 below another lane
    if F >= 2 and row0:
        for i, r in enumerate(row0[:8], start=3):
            c = 1 + (i * 5) % (F - 1)
            reads[i], refs[i] = ord("A"), ord("C")
            reads[i, r - 1], refs[i, c - 1], reads[i, r], refs[i, c] = ord("G"), ord("G"), ord("T"), ord("T")
    return reads, refs


def _engine(monkeypatch, R, F, geometry, plain=False, scoring=SCORING):
    debug_switches(monkeypatch, no_tilt=1 if plain else None)
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*_args(scoring)), group_lanes=geometry[0], rows_per_lane=geometry[1])
    eng.set_half_float_cells(0)
    return eng


def _oracle(alg, reads, refs, scoring=SCORING):
    return cpu_ref.score(alg, reads, refs, cpu_ref.Scoring.make(*_args(scoring)), threads=4, affine=True)


def _check(eng, reads, refs, exp, frame, geometry, what):
    got = eng.score_device(host.SW, _device(reads), _device(refs)).cpu().numpy()
    bad = np.nonzero(got != exp)[0]
    assert not bad.size, what + (frame, bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist())
    d = eng.describe(host.SW, len(reads))
    assert d["ran_score_cells"] == "int16" and d["ran_score_sym_affine"] == "max3", what + (d,)
    assert d["ran_score_sym_affine_frame"] == frame, what + (frame, d["ran_score_sym_affine_frame"])
    assert d["ran_score_geometry"] == "%dx%d" % geometry, what + (d,)


def _shapes(G, K):
    rows = G * K
    leads1, full, leads1_odd = rows - K, rows, rows - 2 * K + 1       # 16x10: 150, 160, 141
    assert (_lead(leads1, G, K), _lead(full, G, K), _lead(leads1_odd, G, K)) == (1, 0, 1)
    out = []
    for R in (leads1, full, leads1_odd):
        widths = [1, 9, 10, 11, 37] if (G, K) == (16, 10) or R == leads1 else [10, 37]
        out += [(R, F) for F in widths + (_remainder_widths(R, G, K) if R == leads1 else [])]
    if (G, K) == (8, 12):
        out.append((96, 25))
    return sorted(set(out))


@pytest.mark.parametrize("geometry", GEOMS, ids=lambda g: "%dx%d" % g)
def test_every_tilted_geometry(monkeypatch, geometry):
    G, K = geometry
    shapes = _shapes(G, K)
    leads1 = G * K - K
    assert {_steps(leads1, F, G, K) % K for R, F in shapes if R == leads1} >= {0, 1, K - 1}
    for R, F in shapes:
        reads, refs = _batch(R, F, G, K, seed=1000 * R + F)
        exp = _oracle(host.SW, reads, refs)
        assert exp[0] == 0 and exp[1] == exp[2] == SCORING[0]
        if F >= 2:
            assert (exp[3:4] == 2 * SCORING[0]).all()
        eng = _engine(monkeypatch, R, F, geometry)
        _check(eng, reads, refs, exp, "tilted", geometry, ("inframe", R, F))
        eng.close()


@pytest.mark.parametrize("gaps", ((-1, -1), (-4, 0), (-7, -3), (0, 0)), ids=lambda g: "open%d-ext%d" % g)
def test_opening_costs_in_the_frame(monkeypatch, gaps):
    """o - x zero, positive and (open above extend is refused) never negative; a mismatch score above zero."""
    for geometry, (R, F) in (((16, 10), (150, 37)), ((8, 12), (96, 25)), ((32, 8), (250, 19))):
        for sub in ((5, -4), (3, 1)):
            scoring = sub + gaps
            reads, refs = _batch(R, F, geometry[0], geometry[1], seed=R + F)
            eng = _engine(monkeypatch, R, F, geometry, scoring=scoring)
            _check(eng, reads, refs, _oracle(host.SW, reads, refs, scoring), "tilted", geometry, ("gaps", scoring))
            eng.close()


@pytest.mark.parametrize("shape", ((16, 10, 150, 2000), (8, 12, 96, 1003), (16, 10, 141, 1501)), ids=lambda s: "%dx%d-%dx%d" % s)
def test_long_references_build_the_profile_from_unstaged_reads(monkeypatch, shape):
    """References too long to stage the wave's pairs in one go: the set-up reads the bases of the reads straight from memory and
    writes the profile score by score -- the other place the row-0 addend is applied."""
    G, K, R, F = shape
    reads, refs = _batch(R, F, G, K, seed=F)
    reads, refs = np.ascontiguousarray(reads[:64]), np.ascontiguousarray(refs[:64])
    eng = _engine(monkeypatch, R, F, (G, K))
    _check(eng, reads, refs, _oracle(host.SW, reads, refs), "tilted", (G, K), ("unstaged", R, F))
    eng.close()


@pytest.mark.parametrize("geometry", ((16, 10), (8, 12)), ids=lambda g: "%dx%d" % g)
def test_the_plain_frame_has_no_addend(monkeypatch, geometry):
    G, K = geometry
    R, F = G * K - K, 37
    reads, refs = _batch(R, F, G, K, seed=5)
    eng = _engine(monkeypatch, R, F, geometry, plain=True)
    _check(eng, reads, refs, _oracle(host.SW, reads, refs), "plain", geometry, ("no_tilt", R, F))
    eng.close()


@pytest.mark.parametrize("geometry", ((16, 10), (8, 12)), ids=lambda g: "%dx%d" % g)
def test_an_nw_score_after_a_tilted_launch(monkeypatch, geometry):
    G, K = geometry
    R, F = G * K - K, 37
    reads, refs = _batch(R, F, G, K, seed=6)
    eng = _engine(monkeypatch, R, F, geometry)
    _check(eng, reads, refs, _oracle(host.SW, reads, refs), "tilted", geometry, ("before NW", R, F))
    got = eng.score_device(host.NW, _device(reads), _device(refs)).cpu().numpy()
    assert np.array_equal(got, _oracle(host.NW, reads, refs))
    _check(eng, reads, refs, _oracle(host.SW, reads, refs), "tilted", geometry, ("after NW", R, F))
    eng.close()
