"""The checkpointed traceback as an algorithm, on the CPU and independent of the kernels: ckpt_align_ref.py (forward fill that
keeps boundary rows, per-strip re-fill limited to the walk's columns, resumable walk carrying the affine state) equals
cpu_ref.align for both algorithms, linear and affine gaps, at strip heights 1, 3, 8 and "taller than the read"."""
import numpy as np
import pytest

from oracle import cpu_ref
from versalignlib_amd import synth
import ckpt_align_ref as car

LINEAR = (2, -1, -3, -2)
AFFINE = (2, -1, -3, -3, -5, -1, -4, -2)
HEIGHTS = [1, 3, 8, 1000]


def _scoring(affine):
    return cpu_ref.Scoring.make(*(AFFINE if affine else LINEAR))


def _check(alg, reads, refs, affine, height, stats=None):
    sc = _scoring(affine)
    exp_rows, exp_idx = cpu_ref.align(alg, reads, refs, sc, threads=2, affine=affine)
    rows, idx = car.align(alg, reads, refs, sc, height, affine=affine, stats=stats)
    bad = [p for p in range(len(reads)) if not (np.array_equal(rows[p], exp_rows[p]) and np.array_equal(idx[p], exp_idx[p]))]
    assert not bad, (alg, affine, height, bad[:8], idx[bad[0]], exp_idx[bad[0]])


def gap_pairs(n=24, R=26, F=34, seed=3):
    """Reads that are their reference with one chunk cut out of the read (a horizontal gap) or of the reference (a vertical
    one), the cut walking over every read row -- so that for every strip height some path crosses a strip boundary inside a
    vertical gap and some path meets a horizontal gap at a boundary row."""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", np.uint8)
    reads, refs = np.zeros((n, R), np.uint8), np.zeros((n, F), np.uint8)
    for p in range(n):
        core = rng.choice(bases, size=R + 8)
        at = 2 + p % (R - 6)
        if p % 2 == 0:                  # the read has 4 bases the reference lacks: UP moves around read row `at`
            read = core[:R]
            ref = np.concatenate([core[:at], core[at + 4:]])
        else:                           # the reference has 5 bases the read lacks: LEFT moves in read row `at`
            ref = core[:R + 5]
            read = np.concatenate([core[:at], core[at + 5:]])[:R]
        reads[p, :len(read)] = read[:R]
        refs[p, :min(len(ref), F)] = ref[:F]
    return reads, refs


def column0_pairs(n=10, R=30, F=9, seed=5):
    """Reads much longer than their reference, the reference matching the read's END: the NW variant's path runs out of
    reference columns (j < 0) many rows above row 0 and goes UP through column 0."""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", np.uint8)
    refs = rng.choice(bases, size=(n, F))
    reads = rng.choice(bases, size=(n, R))
    for p in range(n):
        tail = 4 + p % 5
        reads[p, R - tail:] = refs[p, :tail]
    return reads, refs


@pytest.mark.parametrize("height", HEIGHTS)
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("alg", [car.SW, car.NW])
def test_equals_the_oracle_on_mixed_batches(alg, affine, height):
    for R, F, n, seed in ((17, 23, 24, 1), (33, 12, 16, 2), (8, 40, 16, 3), (1, 1, 4, 4)):
        reads, refs = synth.make_pairs(n, R, F, seed=seed, sub_rate=0.1, indel_rate=0.06, n_run_frac=0.15, short_frac=0.25,
                                       lowercase_frac=0.05, junk_frac=0.05)
        _check(alg, reads, refs, affine, height)


@pytest.mark.parametrize("height", HEIGHTS)
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("alg", [car.SW, car.NW])
def test_gaps_across_strip_boundaries(alg, affine, height):
    reads, refs = gap_pairs()
    stats = {}
    _check(alg, reads, refs, affine, height, stats)
    if height < reads.shape[1]:
        assert stats["paused_in_vertical_gap"] > 0 and stats["horizontal_gap_at_boundary"] > 0, stats
        assert stats["rounds"] > len(reads), stats
    else:                               # taller than the read: one strip, one round per pair, nothing to resume
        assert stats["rounds"] == len(reads) and stats["paused_in_vertical_gap"] == 0, stats


@pytest.mark.parametrize("height", HEIGHTS)
@pytest.mark.parametrize("affine", [False, True])
def test_nw_column_0_above_the_last_strip(affine, height):
    reads, refs = column0_pairs()
    stats = {}
    _check(car.NW, reads, refs, affine, height, stats)
    if height < reads.shape[1]:
        assert stats["column0_above_strip0"] > 0, stats


@pytest.mark.parametrize("affine", [False, True])
def test_short_prefixes_start_in_early_rounds_and_refills_stay_left_of_the_walk(affine):
    """Reads that are short prefixes: end cells in early strips, idle rounds before them -- and a re-fill never sweeps more
    than the columns left of the walk, so the re-filled cells stay below the matrix."""
    R, F, n = 30, 28, 12
    reads, refs = synth.make_pairs(n, R, F, seed=9, sub_rate=0.05, indel_rate=0.02)
    for p in range(n):
        reads[p, (0, 1, 5, 9, 16, 30)[p % 6]:] = 0
    for alg in (car.SW, car.NW):
        stats = {}
        _check(alg, reads, refs, affine, 4, stats)
        assert stats["idle_rounds"] > 0 and 0 < stats["refilled_cells"] < n * R * F, stats
