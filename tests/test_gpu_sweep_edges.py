"""The fixed part of a score sweep at its edges (dp_kernels.hip.h): Smith-Waterman sweeps run without masked fill / drain
steps, from the first lane that owns a real row; wave_setup classifies reference and read bytes a dword at a time
(base_classes.h) and stages the wave's reads in LDS.  Everything is compared EXACTLY with oracle.cpu_ref: shapes where fill and
drain overlap or the step count changes parity, references that end in NUL / N (fewer columns swept than the batch has),
a length-sorted launch with several reference lengths, every byte value at every alignment of the staged spans, a scores
pointer that is not dword-aligned, and compute_alignments for the set-up's first-invalid-base search.  The NW variant
keeps its masked steps: it runs through the same cases as the control."""
import numpy as np
import pytest

from oracle import cpu_ref
from versalignlib_amd import hipkernel, host

from conftest import debug_switches

pytestmark = pytest.mark.gpu

# name -> (arguments of Scoring.make, affine)
SCORINGS = {
    "linear_two_gaps": ((2, -1, -3, -2), False),
    "linear_shared_gap": ((2, -1, -3, -3), False),
    "affine_sym": ((2, -1, -3, -3, -5, -1, -5, -1), True),
    "affine_asym": ((2, -1, -3, -3, -5, -1, -4, -2), True),
}
ALGS = (host.SW, host.NW)

_oracle_cache = {}


def _oracle(key, alg, scoring, reads, refs):
    """cpu_ref.score of a case, computed once and shared by the half-float and the int16 run (read-only)."""
    k = (key, alg, scoring)
    if k not in _oracle_cache:
        args, affine = SCORINGS[scoring]
        exp = cpu_ref.score(alg, reads, refs, cpu_ref.Scoring.make(*args), threads=4, affine=affine)
        exp.setflags(write=False)
        _oracle_cache[k] = exp
    return _oracle_cache[k]


def _engine(R, F, scoring, half):
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*SCORINGS[scoring][0]))
    eng.set_half_float_cells(half)
    return eng


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


def _device(a):
    import torch
    return torch.from_numpy(a).cuda()


# ---- 1. fill and drain overlap, the step count changes parity, tail waves ----
EDGE_F = (1, 2, 15, 16, 17, 31, 32)
EDGE_R = (1, 9, 10, 11, 150, 160)
EDGE_N = (1, 7, 9, 64)


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("scoring", sorted(SCORINGS))
def test_short_sweeps_every_parity_and_tail(scoring, half):
    for R in EDGE_R:
        for F in EDGE_F:
            reads, refs = _related_pairs(max(EDGE_N), R, F, seed=1000 * R + F)
            d_reads, d_refs = _device(reads), _device(refs)
            eng = _engine(R, F, scoring, half)
            for alg in ALGS:
                exp = _oracle(("edge", R, F), alg, scoring, reads, refs)
                for n in EDGE_N:
                    got = eng.score_device(alg, d_reads[:n], d_refs[:n]).cpu().numpy()
                    assert np.array_equal(got, exp[:n]), (R, F, n, alg, np.nonzero(got != exp[:n])[0][:8])
            eng.close()


# ---- 2. references whose tail is NUL or N: fewer columns swept than the batch has ----
def _tailed_refs(n, R, F, seed):
    reads, refs = _related_pairs(n, R, F, seed)
    rng = np.random.default_rng(seed + 1)
    keep = rng.integers(0, F + 1, size=n)
    for i in range(n):
        refs[i, keep[i]:] = 0 if i % 3 else ord("N") if i % 2 else ord("n")
    refs[0:8] = ord("N")                 # a whole wave of all-N references: nothing swept, score 0
    refs[8:16, 3:] = 0                   # a wave that sweeps three columns ...
    refs[13] = _related_pairs(1, R, F, seed + 2)[1][0]      # ... but for one pair with a full-length reference
    refs[16:24, :] = 0                   # nothing but padding
    reads[24] = 0
    reads[25] = ord("N")
    return reads, refs


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("scoring", sorted(SCORINGS))
@pytest.mark.parametrize("R,F", [(150, 500), (33, 70), (10, 17)])
def test_reference_tails_of_nul_and_n(R, F, scoring, half):
    n = 67
    reads, refs = _tailed_refs(n, R, F, seed=7 * R + F)
    d_reads, d_refs = _device(reads), _device(refs)
    eng = _engine(R, F, scoring, half)
    for alg in ALGS:
        exp = _oracle(("tails", R, F), alg, scoring, reads, refs)
        got = eng.score_device(alg, d_reads, d_refs).cpu().numpy()
        assert np.array_equal(got, exp), (alg, np.nonzero(got != exp)[0][:8])
        if alg == host.SW:
            assert not exp[0:8].any() and not exp[16:24].any() and exp[13] > 0
    eng.close()


# ---- 3. a length-sorted launch: three groups of different reference lengths in one sweep ----
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("scoring", sorted(SCORINGS))
def test_length_sorted_launch_with_three_reference_lengths(monkeypatch, scoring, half):
    debug_switches(monkeypatch, ragged_min=64)          # read at engine creation: bins at test sizes
    R, F, n = 150, 500, 768
    reads, refs = _related_pairs(n, R, F, seed=31)
    for i, length in enumerate((93, 250, 500)):         # three trimmed lengths, 256 pairs each, interleaved
        refs[i::3, length:] = 0
    d_reads, d_refs = _device(reads), _device(refs)
    eng = _engine(R, F, scoring, half)
    eng.set_ragged_batching(2)
    for alg in ALGS:
        exp = _oracle(("ragged", R, F), alg, scoring, reads, refs)
        got = eng.score_device(alg, d_reads, d_refs).cpu().numpy()
        assert np.array_equal(got, exp), (alg, np.nonzero(got != exp)[0][:8])
        info = eng.describe(alg, n)
        assert info["ragged_launches"] >= 1 and info["ragged_cell_fraction"] < 0.75, info
    eng.close()


# ---- 4. every byte value at every position mod 16 of a reference and of a read, at every alignment of the spans ----
def _byte_value_pairs(R, F, seed):
    """32 pairs: pair p carries byte values 8 p .. 8 p + 7 -- in pairs 0..15 cycling along the READ, in pairs 16..31 (values
    again from 0) along the REFERENCE, so that with 16 start offsets of the buffers every value meets every position
    mod 16.  The other sequence of the pair is letters of both cases."""
    reads, refs = _related_pairs(64, R, F, seed)
    rng = np.random.default_rng(seed + 5)
    lower = rng.random(reads.shape) < 0.5
    reads[lower] |= 0x20
    lower = rng.random(refs.shape) < 0.5
    refs[lower] |= 0x20
    for p in range(32):
        vals = (8 * p + np.arange(8)).astype(np.uint8)
        reads[p] = vals[(np.arange(R) + p) % 8]
        # keep something to score against: the reference repeats the letters among the values (if any), both cases
        refs[32 + p] = vals[(np.arange(F) + p) % 8]
    return reads, refs


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("F", [501, 503])
def test_every_byte_value_at_every_alignment(F, half):
    import torch
    R, n = 149, 64
    reads, refs = _byte_value_pairs(R, F, seed=F)
    # all 256 values occur in the reads and in the references
    assert len(np.unique(reads)) == 256 and len(np.unique(refs)) == 256
    rbuf = torch.zeros(n * R + 64, dtype=torch.uint8, device="cuda")
    fbuf = torch.zeros(n * F + 64, dtype=torch.uint8, device="cuda")
    flat_reads, flat_refs = _device(reads.reshape(-1)), _device(refs.reshape(-1))
    for scoring in ("linear_shared_gap", "affine_sym"):
        eng = _engine(R, F, scoring, half)
        for alg in ALGS:
            exp = _oracle(("bytes", R, F), alg, scoring, reads, refs)
            for ofs in range(16):           # the read span starts at byte `ofs`, the reference span at byte 15 - ofs (mod 16)
                rbuf[ofs:ofs + n * R] = flat_reads
                fbuf[15 - ofs:15 - ofs + n * F] = flat_refs
                got = eng.score_device(alg, rbuf[ofs:ofs + n * R].view(n, R), fbuf[15 - ofs:15 - ofs + n * F].view(n, F)).cpu().numpy()
                assert np.array_equal(got, exp), (scoring, alg, ofs, np.nonzero(got != exp)[0][:8])
        eng.close()


# ---- 5. a scores pointer offset by one element (the pairs of a lane group are no longer one aligned dword) ----
@pytest.mark.parametrize("half", [0, 1])
def test_scores_pointer_offset_by_one_element(half):
    import torch
    R, F, n = 150, 500, 131
    reads, refs = _related_pairs(n, R, F, seed=77)
    d_reads, d_refs = _device(reads), _device(refs)
    for scoring in ("linear_two_gaps", "affine_sym"):
        eng = _engine(R, F, scoring, half)
        for alg in ALGS:
            exp = _oracle(("offset", R, F), alg, scoring, reads, refs)
            out = torch.full((n + 2,), -12345, dtype=torch.int16, device="cuda")
            eng.score_device(alg, d_reads, d_refs, scores=out[1:n + 1])
            got = out.cpu().numpy()
            assert np.array_equal(got[1:n + 1], exp), (scoring, alg)
            assert got[0] == -12345 and got[n + 1] == -12345
        eng.close()


# ---- 6. compute_alignments: the fill kernels' set-up also looks for the first invalid base of a read / a reference ----
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("policy", [0, 1])
def test_alignments_with_invalid_bases_at_every_alignment(alg, policy):
    R, F, n = 149, 501, 64
    reads, refs = _related_pairs(n, R, F, seed=91)
    rng = np.random.default_rng(92)
    junk = np.frombuffer(b"N\x00nXx-*\xc1", dtype=np.uint8)
    for i in range(n):                  # the first invalid base of pair i: position i + k of the read, 3 i + k of the reference
        if i % 4 != 3:
            reads[i, min(R - 1, i + i % 5)::7] = junk[rng.integers(0, len(junk))]
        if i % 4 != 2:
            refs[i, min(F - 1, 3 * i + i % 3)::11] = junk[rng.integers(0, len(junk))]
    refs[5, 200:] = 0
    reads[6, 100:] = 0
    exp_rows, exp_idx = cpu_ref.align(alg, reads, refs, cpu_ref.Scoring.make(), threads=4, policy="sse" if policy else "default")
    eng = hipkernel.Engine(R, F)
    eng.set_traceback_policy(policy)
    rows, idx = eng.align_device(alg, _device(reads), _device(refs))
    rows, idx = rows.cpu().numpy(), idx.cpu().numpy()
    eng.close()
    assert np.array_equal(idx, exp_idx), np.nonzero((idx != exp_idx).any(axis=1))[0][:8]
    assert np.array_equal(rows, exp_rows), np.nonzero((rows != exp_rows).reshape(n, -1).any(axis=1))[0][:8]
