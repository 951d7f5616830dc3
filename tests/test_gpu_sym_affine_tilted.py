"""The two frames of the biased int16 Smith-Waterman sweep with symmetric affine gaps (score_kernel<G, K, kAlgSW,
kGapAffineSym>, dp_kernels.hip.h): inside its window and on geometries of at most 12 rows per lane the engine launches the
biased form in a TILTED frame, in which a gap extension costs nothing (tests/test_sym_affine_tilted_sweep.py restates it on
the CPU); beyond that window, on the taller geometries, or under VALIGN_HIP_DEBUG=no_tilt, the plain frame.  Everything here
runs on int16 cells (set_half_float_cells(0)), is compared EXACTLY with oracle.cpu_ref.score, runs both frames and asserts
through describe() which one ran (ran_score_sym_affine stays "max3" for both):

  a. one-hot batches in which a single cell can supply the score, at every (row, column), on 16x10, 8x12 and 32x8, at reference
     widths whose step counts leave 0, 1 and K - 1 remainder steps in front of the K-step trips;
  b. random related pairs with long insertions and deletions over the (open, extend) pairs and substitution scores of
     tests/test_gpu_sym_affine_max3.py, and a batch with N runs and NUL-padded short pairs;
  c. the tilted window's upper edge on 16x10: the last match score that runs tilted, the first that runs plain (still "max3");
  d. a length-sorted batch, identical to the padded sweep;
  e. a geometry of 16 rows per lane runs the plain frame."""
import numpy as np
import pytest

from conftest import debug_switches
from oracle import cpu_ref
from test_gpu_sym_affine_max3 import GAPS, _args, _device, _gapped_pairs, _one_hot, _refused
from versalignlib_amd import hipkernel, host

pytestmark = pytest.mark.gpu

FRAMES = ("tilted", "plain")

_oracle_cache = {}


def _oracle(key, scoring, reads, refs):
    """cpu_ref.score of a case, computed once and shared by both frames (read-only)."""
    k = (key, scoring)
    if k not in _oracle_cache:
        exp = cpu_ref.score(host.SW, reads, refs, cpu_ref.Scoring.make(*_args(scoring)), threads=4, affine=True)
        exp.setflags(write=False)
        _oracle_cache[k] = exp
    return _oracle_cache[k]


def _engine(monkeypatch, R, F, scoring, geometry=None, frame="tilted"):
    """An int16 engine; frame "plain" forces the plain frame with the debug switch (read when the engine is created)."""
    debug_switches(monkeypatch, no_tilt=1 if frame == "plain" else None)
    G, K = geometry or (0, 0)
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*_args(scoring)), group_lanes=G, rows_per_lane=K)
    eng.set_half_float_cells(0)
    return eng


def _check(eng, d_reads, d_refs, exp, frame, geometry, what):
    n = int(d_reads.shape[0])
    got = eng.score_device(host.SW, d_reads, d_refs).cpu().numpy()
    bad = np.nonzero(got != exp[:n])[0]
    assert not bad.size, what + (frame, bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist())
    d = eng.describe(host.SW, n)
    assert d["ran_score_cells"] == "int16", what + (d,)
    assert d["ran_score_sym_affine"] == "max3", what + (d["ran_score_sym_affine"],)
    assert d["ran_score_sym_affine_frame"] == frame, what + (frame, d["ran_score_sym_affine_frame"])
    if geometry:
        assert d["ran_score_geometry"] == "%dx%d" % geometry, what + (d,)


def _steps(R, F, G, K):
    rows = G * K
    return F + G - 1 - ((rows - R) // K if rows > R else 0)


# ---- a. one matching base at (row i, column j): widths with steps % K = 0, 1, K - 1 ----
@pytest.mark.parametrize("shape", ((150, (16, 17, 15), 16, 10), (96, (17, 18, 16), 8, 12), (250, (9, 10, 8), 32, 8)),
                         ids=lambda s: "%d-on-%dx%d" % (s[0], s[2], s[3]))
def test_one_matching_base_at_every_cell(monkeypatch, shape):
    R, widths, G, K = shape
    scoring = (2, -1, -5, -1)
    assert [_steps(R, F, G, K) % K for F in widths] == [0, 1, K - 1] and all(8 <= F <= 24 for F in widths)
    for width in widths:
        reads, refs = _one_hot(R, width)
        d_reads, d_refs = _device(reads), _device(refs)
        exp = _oracle(("one_hot", R, width), scoring, reads, refs)
        assert (exp == scoring[0]).all()                   # the match score, from the one cell that has it
        for frame in FRAMES:
            eng = _engine(monkeypatch, R, width, scoring, (G, K), frame)
            _check(eng, d_reads, d_refs, exp, frame, (G, K), ("one_hot", R, width))
            eng.close()


# ---- b. long gaps in both directions; bases that score nothing ----
@pytest.mark.parametrize("shape", ((150, 64), (37, 5)), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("gaps", GAPS)
def test_long_gaps_in_both_directions(monkeypatch, gaps, shape):
    R, F = shape
    reads, refs = _gapped_pairs(600, R, F, seed=1000 * R + F)
    d_reads, d_refs = _device(reads), _device(refs)
    for sub in ((2, -1), (5, -4)):
        scoring = sub + gaps
        if _refused(scoring):
            return
        exp = _oracle(("gapped", R, F), scoring, reads, refs)
        for frame in FRAMES:
            eng = _engine(monkeypatch, R, F, scoring, None, frame)
            _check(eng, d_reads, d_refs, exp, frame, None, ("gapped", R, F, scoring))
            eng.close()


def test_n_runs_and_short_pairs(monkeypatch):
    """Bases that score nothing inside the pairs (N runs) and behind them (NUL-padded short reads and references): the zero
    slab, which carries 2x in the tilted frame, ragged columns, waves whose pairs end at different columns."""
    R, F, n = 150, 64, 600
    reads, refs = _gapped_pairs(n, R, F, seed=7)
    rng = np.random.default_rng(8)
    for i in range(n):
        if i % 3 == 0:
            a = int(rng.integers(0, F - 8))
            refs[i, a:a + int(rng.integers(1, 9))] = ord("N")
        if i % 4 == 0:
            a = int(rng.integers(0, R - 12))
            reads[i, a:a + int(rng.integers(1, 13))] = ord("N")
        if i % 2 == 1:
            refs[i, int(rng.integers(1, F)):] = 0
        if i % 5 == 2:
            reads[i, int(rng.integers(1, R)):] = 0
    d_reads, d_refs = _device(reads), _device(refs)
    for scoring in ((2, -1, -5, -1), (5, -4, -4, 0)):
        exp = _oracle(("n_runs", R, F), scoring, reads, refs)
        for frame in FRAMES:
            eng = _engine(monkeypatch, R, F, scoring, None, frame)
            _check(eng, d_reads, d_refs, exp, frame, None, ("n_runs", scoring))
            eng.close()


# ---- c. the tilted window's upper edge, from the rule: B + x * (rows + F - lead) + 64 * match + 1 <= 0x7BFF ----
def _tilted_edge(R, F, G, K, mismatch, gap_open, gap_ext):
    """The last match score the rule (cell_rules.h: sym_affine_tilt_ok) lets run tilted."""
    o, x, rows = -gap_open, -gap_ext, G * K
    B = 1024 + max(o - x, -mismatch, 0)
    top = rows + F - ((rows - R) // K if rows > R else 0)
    return (0x7BFF - B - x * top - 1) // min(R, F)


@pytest.mark.parametrize("beyond", (0, 1), ids=("last-tilted", "first-plain"))
def test_the_tilted_windows_upper_edge(monkeypatch, beyond):
    R, F, n = 150, 64, 40
    match = _tilted_edge(R, F, 16, 10, -1, -5, -1) + beyond
    assert 1031 + 64 * match + 1 <= 0x7BFF                          # inside the plain biased form's window either way
    rng = np.random.default_rng(match)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = np.ascontiguousarray(acgt[rng.integers(0, 4, size=(n, R))])
    # the reference is the read's LAST 64 bases: the full score is reached in the last rows at the last columns, where the tilt
    # is largest
    refs = np.ascontiguousarray(reads[:, R - F:])
    refs[n // 2:, 20] = ord("N")                                    # ... half of them one base short of the full score
    scoring = (match, -1, -5, -1)
    exp = _oracle(("edge", match), scoring, reads, refs)
    assert (exp[:n // 2] == 64 * match).all() and exp.max() == 64 * match <= 32767
    eng = _engine(monkeypatch, R, F, scoring, (16, 10))
    _check(eng, _device(reads), _device(refs), exp, "plain" if beyond else "tilted", (16, 10), ("edge", match))
    eng.close()


# ---- d. length-sorted batches sweep packed groups with one launch each; the frame is the engine's ----
def test_length_sorted_batch(monkeypatch):
    R, F, n = 150, 64, 300
    reads, refs = _gapped_pairs(n, R, F, seed=11)
    rng = np.random.default_rng(12)
    for i in range(n):                                             # ragged: references of 8 to 64 bases, reads of 30 to 150
        refs[i, int(rng.integers(8, F + 1)):] = 0
        reads[i, int(rng.integers(30, R + 1)):] = 0
    d_reads, d_refs = _device(reads), _device(refs)
    scoring = (2, -1, -5, -1)
    exp = _oracle(("sorted", R, F), scoring, reads, refs)
    debug_switches(monkeypatch, ragged_min=32)                     # (read at engine creation: length bins at this batch size)
    for frame in FRAMES:
        eng = _engine(monkeypatch, R, F, scoring, None, frame)
        padded = eng.score_device(host.SW, d_reads, d_refs).cpu().numpy()
        eng.set_ragged_batching(2)
        _check(eng, d_reads, d_refs, exp, frame, None, ("sorted",))
        assert eng.describe(host.SW, n)["ragged_launches"] >= 1     # the length classes were swept, not the padded batch
        assert np.array_equal(padded, exp)
        eng.close()


# ---- e. 16 rows per lane: the K-step trip is not built, the plain frame runs ----
def test_tall_geometry_runs_the_plain_frame(monkeypatch):
    R, F = 150, 64
    reads, refs = _gapped_pairs(200, R, F, seed=21)
    scoring = (2, -1, -5, -1)
    exp = _oracle(("tall", R, F), scoring, reads, refs)
    eng = _engine(monkeypatch, R, F, scoring, (64, 16))
    _check(eng, _device(reads), _device(refs), exp, "plain", (64, 16), ("tall",))
    eng.close()
