"""The tilted frame of the biased int16 Smith-Waterman sweep with symmetric affine gaps (score_kernel<G, K, kAlgSW,
kGapAffineSym>, dp_kernels.hip.h) around the first lane's padding rows, with the slab numbers of a step fetched as single
LDS bytes in the trips and in the remainder tail.  The geometries 16 x 10, 8 x 12 and 32 x 8 are forced as
tests/test_gpu_sym_affine_inframe.py forces them, on int16 cells, and compared EXACTLY with oracle.cpu_ref.score:

  reads that leave 0, 1, K - 1, K and K + 1 padding rows (16 x 10: 160, 159, 151, 150 and 149 bases: the read's first base
  in the first lane's row 0, its row 1, its last row, in the second lane's row 0 and in its row 1) against references of
  K + 1 and 37 bases.  Each batch is that file's -- gapped related pairs, a read that scores nothing, one matching base on
  the first and on the last anti-diagonal, a diagonal across a lane boundary -- plus pairs whose only matching base is the
  read's FIRST base, against column 0 and against column F - 1: the cell whose diagonal is the last padding row (with K
  padding rows: the lane hand-over of it, with none: the moving border), and one pair whose first two read bases match in
  a row."""
import pytest

from test_gpu_sym_affine_inframe import SCORING, _batch, _check, _engine, _oracle
from versalignlib_amd import host

pytestmark = pytest.mark.gpu

GEOMS = ((16, 10), (8, 12), (32, 8))
FIRST = 12                                                            # the first pair of this file's own (the other file's: 0 .. 10)


def _paddings(K):
    return (0, 1, K - 1, K, K + 1)


def _first_base_batch(R, F, G, K, seed):
    reads, refs = _batch(R, F, G, K, seed)
    for i, cols in ((FIRST, (0,)), (FIRST + 1, (F - 1,)), (FIRST + 2, (F // 2, F // 2 + 1))):
        reads[i], refs[i] = ord("A"), ord("C")
        for r, c in enumerate(cols):                                  # read base r against column c, nothing else matches
            reads[i, r], refs[i, c] = b"GT"[r], b"GT"[r]
    return reads, refs


@pytest.mark.parametrize("geometry", GEOMS, ids=lambda g: "%dx%d" % g)
def test_with_and_without_a_padding_row(monkeypatch, geometry):
    G, K = geometry
    assert (G, K) != (16, 10) or [G * K - p for p in _paddings(K)] == [160, 159, 151, 150, 149]
    for pad in _paddings(K):
        R = G * K - pad
        for F in (K + 1, 37):
            reads, refs = _first_base_batch(R, F, G, K, seed=1000 * R + F)
            exp = _oracle(host.SW, reads, refs)
            assert exp[0] == 0 and exp[FIRST] == exp[FIRST + 1] == SCORING[0] and exp[FIRST + 2] == 2 * SCORING[0]
            eng = _engine(monkeypatch, R, F, geometry)
            _check(eng, reads, refs, exp, "tilted", geometry, ("padding", pad, R, F))
            eng.close()


def test_open_and_extend_zero(monkeypatch):
    """o + x = 0 and a mismatch score above zero: every floor is B."""
    scoring = (3, 1, 0, 0)
    for geometry in GEOMS:
        G, K = geometry
        for pad in (0, 1, K):
            R, F = G * K - pad, K + 1
            reads, refs = _first_base_batch(R, F, G, K, seed=R + F)
            eng = _engine(monkeypatch, R, F, geometry, scoring=scoring)
            _check(eng, reads, refs, _oracle(host.SW, reads, refs, scoring), "tilted", geometry, ("zero gaps", pad, R, F))
            eng.close()
