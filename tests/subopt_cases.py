"""Inputs the CPU and the GPU tests of the suboptimal scores share: planted batches whose runner-up the construction states."""
import numpy as np

BASES = np.frombuffer(b"ACGT", np.uint8)


def random_bases(rng, shape):
    return BASES[rng.integers(0, 4, shape)]


def mutate(seq, positions):
    """a copy of seq with the bases at `positions` replaced by another base"""
    out = seq.copy()
    for p in positions:
        out[p] = BASES[(int(np.searchsorted(BASES, out[p])) + 1) % 4]
    return out


def planted(n, R, F, seed, read_len=None, at=10, pad=0, second_at=None, second_mismatches=3):
    """n pairs: a read of read_len random bases (padded to R with `pad`) planted in a random reference at column `at`; with
    second_at, a copy with `second_mismatches` spread mismatches at that column too."""
    rng = np.random.default_rng(seed)
    L = R if read_len is None else read_len
    reads = np.full((n, R), pad, np.uint8)
    refs = random_bases(rng, (n, F))
    for p in range(n):
        rd = random_bases(rng, L)
        reads[p, :L] = rd
        refs[p, at:at + L] = rd
        if second_at is not None:
            where = [(k + 1) * L // (second_mismatches + 1) for k in range(second_mismatches)]
            refs[p, second_at:second_at + L] = mutate(rd, where)
    return reads, refs


def fuzz_batch(n, R, F, seed, plant_at=10):
    """Half of the reads planted at column plant_at (the generator of the issue: R = 33, F = 70, mask = 16), the rest random;
    ragged tails on a quarter of reads and references (NUL or N)."""
    rng = np.random.default_rng(seed)
    reads = random_bases(rng, (n, R))
    refs = random_bases(rng, (n, F))
    planted_rows = np.arange(n) % 2 == 0
    span = min(R, F - plant_at)
    if span > 0:
        refs[planted_rows, plant_at:plant_at + span] = reads[planted_rows, :span]
    for p in range(n):
        if rng.random() < 0.25 and R > 4:
            reads[p, rng.integers(R // 2, R):] = rng.choice([0, ord("N")])
        if rng.random() < 0.25 and F > 4:
            refs[p, rng.integers(F // 2, F):] = rng.choice([0, ord("N")])
    return reads, refs, planted_rows
