"""The two forms of the int16 Smith-Waterman sweep with symmetric affine gaps (score_kernel<G, K, kAlgSW, kGapAffineSym>,
dp_kernels.hip.h): inside its window the engine launches the biased form, whose maxima go three at a time through the packed
half-float maximum on cells kept as value + B (tests/test_sym_affine_max3_sweep.py restates it on the CPU); beyond the window,
or under VALIGN_HIP_DEBUG=no_max3, the gap-source form.  Everything here runs on int16 cells (set_half_float_cells(0)), is
compared EXACTLY with oracle.cpu_ref.score, and asserts through describe() which form ran:

  1. one-hot batches in which a single cell can supply the score, at every (row, column) -- an odd and an even step count, the
     lanes above the sweep's first lane, the last lane -- on 16x10, 8x12 and 32x8 (whose hand-over between lanes is a wave
     shift with the border merged in behind it, not a DPP row shift), each with the default form and with no_max3;
  2. random related pairs with long insertions and deletions over the (open, extend) pairs of tests/test_gpu_sym_affine_sweep.py,
     and a batch with N runs and NUL-padded short pairs (ragged columns, the zero slab);
  3. the window's upper edge on 16x10: the last match score that runs the biased form, the first that does not, and the last one
     int16 cells hold at all;
  4. a length-sorted batch, identical to the padded sweep.

(open, extend) = (-2, -3) is no affine model and the engine refuses it at construction: its cases check exactly that."""
import numpy as np
import pytest

from conftest import debug_switches
from oracle import cpu_ref
from versalignlib_amd import hipkernel, host

pytestmark = pytest.mark.gpu

GAPS = ((-5, -1), (-1, -1), (-2, -3), (-4, 0), (0, 0))          # (open, extend), the same for both directions
FORMS = ("max3", "sources")

_oracle_cache = {}


def _args(scoring):
    match, mismatch, gap_open, gap_ext = scoring
    return (match, mismatch, -3, -3, gap_open, gap_ext, gap_open, gap_ext)


def _oracle(key, scoring, reads, refs):
    """cpu_ref.score of a case, computed once and shared by both forms (read-only)."""
    k = (key, scoring)
    if k not in _oracle_cache:
        exp = cpu_ref.score(host.SW, reads, refs, cpu_ref.Scoring.make(*_args(scoring)), threads=4, affine=True)
        exp.setflags(write=False)
        _oracle_cache[k] = exp
    return _oracle_cache[k]


def _refused(scoring):
    if scoring[3] >= scoring[2]:
        return False
    with pytest.raises(hipkernel.HipKernelError, match="extend >= open"):
        hipkernel.Engine(150, 64, hipkernel.Scoring.make(*_args(scoring)))
    return True


def _engine(monkeypatch, R, F, scoring, geometry=None, form="max3"):
    """An int16 engine; form "sources" forces the gap-source form with the debug switch (read when the engine is created)."""
    debug_switches(monkeypatch, no_max3=1 if form == "sources" else None)
    G, K = geometry or (0, 0)
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*_args(scoring)), group_lanes=G, rows_per_lane=K)
    eng.set_half_float_cells(0)
    return eng


def _check(eng, d_reads, d_refs, exp, form, geometry, what):
    n = int(d_reads.shape[0])
    got = eng.score_device(host.SW, d_reads, d_refs).cpu().numpy()
    bad = np.nonzero(got != exp[:n])[0]
    assert not bad.size, what + (form, bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist())
    d = eng.describe(host.SW, n)
    assert d["ran_score_cells"] == "int16", what + (d,)
    assert d["ran_score_sym_affine"] == form, what + (form, d["ran_score_sym_affine"])
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


@pytest.mark.parametrize("shape", ((150, 23, 16, 10), (96, 9, 8, 12), (250, 11, 32, 8)), ids=lambda s: "%dx%d-on-%dx%d" % s)
def test_one_matching_base_at_every_cell(monkeypatch, shape):
    R, F, G, K = shape
    scoring = (2, -1, -5, -1)
    for width in (F, F - 1):                              # both parities of the step count
        reads, refs = _one_hot(R, width)
        d_reads, d_refs = _device(reads), _device(refs)
        exp = _oracle(("one_hot", R, width), scoring, reads, refs)
        assert (exp == scoring[0]).all()                   # the match score, from the one cell that has it
        for form in FORMS:
            eng = _engine(monkeypatch, R, width, scoring, (G, K), form)
            _check(eng, d_reads, d_refs, exp, form, (G, K), ("one_hot", R, width))
            eng.close()


# ---- 2. reads with pieces of 1 to 12 bases deleted or inserted against their reference: long gaps in both directions ----
def _gapped_pairs(n, R, F, seed):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    refs = acgt[rng.integers(0, 4, size=(n, F))]
    reads = acgt[rng.integers(0, 4, size=(n, R))]                   # (what a short reference does not fill stays random)
    for i in range(n):
        out, pos = [], int(rng.integers(0, max(1, F // 4)))
        while sum(len(p) for p in out) < R and pos < F:
            run = int(rng.integers(4, 30))
            out.append(refs[i, pos:pos + run])
            pos += run
            gap = int(rng.integers(1, 13))
            if rng.random() < 0.5:
                pos += gap                                              # deleted from the read
            else:
                out.append(acgt[rng.integers(0, 4, size=gap)])          # inserted into the read
        piece = np.concatenate(out)[:R]
        reads[i, :len(piece)] = piece
    return np.ascontiguousarray(reads), np.ascontiguousarray(refs)


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
        if shape == (150, 64) and gaps == (-5, -1) and sub == (2, -1):
            assert (exp > 29 * sub[0]).mean() > 0.5         # the gaps are used: no ungapped piece of a read has 30 bases
        for form in FORMS:
            eng = _engine(monkeypatch, R, F, scoring, None, form)
            _check(eng, d_reads, d_refs, exp, form, None, ("gapped", R, F, scoring))
            eng.close()


def test_n_runs_and_short_pairs(monkeypatch):
    """Bases that score nothing inside the pairs (N runs) and behind them (NUL-padded short reads and references): the zero
    slab, ragged columns, waves whose pairs end at different columns."""
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
        for form in FORMS:
            eng = _engine(monkeypatch, R, F, scoring, None, form)
            _check(eng, d_reads, d_refs, exp, form, None, ("n_runs", scoring))
            eng.close()


# ---- 3. the window's upper edge: B = 1024 + 5 + 1 + 1 = 1031, hi = 64 * match + 1, the form is legal while B + hi <= 0x7BFF ----
@pytest.mark.parametrize("match, form", ((479, "max3"), (480, "sources"), (499, "sources")))
def test_the_windows_upper_edge(monkeypatch, match, form):
    R, F, n = 150, 64, 40
    rng = np.random.default_rng(match)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = np.ascontiguousarray(acgt[rng.integers(0, 4, size=(n, R))])
    refs = np.ascontiguousarray(reads[:, :F])                      # the reference is the read's first 64 bases
    refs[n // 2:, 20] = ord("N")                                    # ... half of them one base short of the full score
    scoring = (match, -1, -5, -1)
    assert 1031 + 64 * match + 1 <= 0x7BFF if form == "max3" else 1031 + 64 * match + 1 > 0x7BFF
    exp = _oracle(("edge", match), scoring, reads, refs)
    assert (exp[:n // 2] == 64 * match).all() and exp.max() == 64 * match <= 32767
    eng = _engine(monkeypatch, R, F, scoring, (16, 10))
    _check(eng, _device(reads), _device(refs), exp, form, (16, 10), ("edge", match))
    eng.close()


# ---- 4. length-sorted batches sweep packed groups with one launch each; the form is the engine's ----
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
    for form in FORMS:
        eng = _engine(monkeypatch, R, F, scoring, None, form)
        padded = eng.score_device(host.SW, d_reads, d_refs).cpu().numpy()
        eng.set_ragged_batching(2)
        _check(eng, d_reads, d_refs, exp, form, None, ("sorted",))
        assert eng.describe(host.SW, n)["ragged_launches"] >= 1     # the length classes were swept, not the padded batch
        assert np.array_equal(padded, exp)
        eng.close()
