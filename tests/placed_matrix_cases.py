"""The inputs of tests/test_gpu_placed_matrix.py and their references, shared with tests/test_instance_matrix_table.py, which
holds the inputs against the conditions below on the CPU.  No GPU and no library here: numpy and tests/placed_ref.py.

A case is (G, K, R, F) of instance_matrix -- a forced geometry at one of its four shapes -- with instance_matrix.batch(G)
pairs of two kinds:

  random related pairs (about two thirds; half of the ten pairs a 64-lane geometry gets): built as test_gpu_placed._pairs builds
  them -- substitutions, indels, N runs, NUL-trimmed tails, lower case, junk bytes -- then each read rotated by a random number of
  rows, so that the best alignments end in every part of the register and not all near row F, and every other read trimmed to a
  random length with NUL or N, so that the two halves of a packed register differ in their padding rows;

  planted two-cell ties (the rest, at least five): all-N pairs with read[r1] = A, read[r2] = C, ref[c1] = C, ref[c2] = A, r1 < r2,
  c1 < c2.  The cells (r1, c2) and (r2, c1) are the only ones where two bases meet and match; an N scores 0 against anything, so
  the diagonals below the two cells carry the same value on, through later rows.  The first cell in row-major order that holds
  the maximum is (r1, c2): the earlier row wins although its column is the later one, whatever the gap form (a single-base match
  scores `match` under affine gaps too; every gap or mismatch step takes something off).  The record (match, r1 + 1, c2 + 1)
  follows from the construction alone.  One pair has the tie in ONE row, read[r] = A, ref[c1] = ref[c2] = A: the first column wins.

The register rows of a forced G x K at R rows are the read's rows below pad = G K - R rows of padding (placed_kernels.hip.h: "the
geometry's pad rows lie on top"): read row r sits in lane (r + pad) // K.  (r1, r2) are placed at: row 0 and row R - 1; rows
K - 2 and K - 1 (two rows of lane 0 at R = G K; at R = G K - K - 1 the last row of the partly padded lane and the first row of
the next one); the first and the last row of one lane; the last row of a lane and the first of the next -- lanes taken from those
that hold no padding row."""
import functools
import types

import numpy as np

import instance_matrix as im
import placed_ref
from versalignlib_amd import synth

# test_gpu_placed.FORMS (the GPU test asserts that they are the same): linear symmetric, linear gap_read != gap_ref, affine
# symmetric, affine with four scores; and the kernel's gap form each one selects
FORMS = {"sym": (-3, -3), "lin": (-2, -4), "affsym": (-3, -3, -5, -1, -5, -1), "aff": (-3, -3, -6, -2, -4, -1)}
FORM_NAMES = {"sym": "Sym", "lin": "Linear", "affsym": "AffineSym", "aff": "Affine"}
TRACKS = ("key", "rows")
# what test_gpu_placed._pairs passes to synth.make_pairs
PAIR_ARGS = dict(sub_rate=0.1, indel_rate=0.02, n_run_frac=0.1, short_frac=0.1, lowercase_frac=0.05, junk_frac=0.04)
MIN_PLANTED = 5

CASES = [(G, K, R, F) for G, K in sorted(im.GEOMETRIES) for R, F in im.shapes(G, K)]


def tracks(K):
    return TRACKS if K <= im.PLACED_KEY_MAX_K else ("rows",)


def rows_match(R, F, K):
    """the smallest match score beyond the lane key's range (placed_choice: (min(R, F) match + 1) << bits > 32000), as
    test_gpu_subopt._rows_match has it; still inside int16"""
    bits = im.placed_key_bits(K)
    m = 32000 // (min(R, F) << bits) + 1
    assert ((min(R, F) * m + 1) << bits) > 32000 and ((min(R, F) * (m - 1) + 1) << bits) <= 32000 and min(R, F) * m + 1 <= 32000
    return m


def scoring_args(track, form, R, F, K):
    """arguments of Scoring.make: match 2 / mismatch -1 on the key track, the first match beyond the key on the rows track"""
    match = 2 if track == "key" else rows_match(R, F, K)
    return (match, -1 if track == "key" else -(match // 2)) + FORMS[form]


def _scoring(args):
    names = ("match", "mismatch", "gap_read", "gap_ref", "open_read", "ext_read", "open_ref", "ext_ref")
    return types.SimpleNamespace(**dict(zip(names, args + (0,) * (len(names) - len(args)))))


def _tie_rows(G, K, R, count):
    """`count` row pairs (r1, r2): the four kinds of the module's text, the lane kinds on one lane after the other"""
    pad = G * K - R
    first_lane = (pad + K - 1) // K                     # the first lane without a padding row
    out = [(0, R - 1), (K - 2, K - 1)]
    span = G - 1 - first_lane                           # lanes first_lane .. G - 2: the next lane exists
    k = 0
    while len(out) < count:
        top = (first_lane + (3 * k + 1) % span) * K - pad
        out.append((top, top + K - 1))                                # first and last row of a lane
        if len(out) < count:
            top = (first_lane + (3 * k + 2 + span // 2) % span) * K - pad
            out.append((top + K - 1, top + K))                        # the last row of a lane and the first of the next
        k += 1
    assert all(0 <= r1 < r2 < R for r1, r2 in out), (G, K, R, out)
    return out


@functools.lru_cache(maxsize=None)
def batch(G, K, R, F):
    """-> reads, refs (read-only), the indices of the random pairs, {index of a planted pair: (read_end, ref_end) by construction}"""
    n = im.batch(G)
    n_planted = max(MIN_PLANTED, n - (2 * n + 1) // 3)
    n_random = n - n_planted
    seed = 7 * R + 131 * F + K
    rng = np.random.default_rng(seed)
    planted_at = [(i * n) // n_planted + (n // n_planted) // 2 for i in range(n_planted)]
    random_at = [p for p in range(n) if p not in set(planted_at)]
    assert len(set(planted_at)) == n_planted and len(random_at) == n_random and max(planted_at) < n
    reads, refs = np.full((n, R), ord("N"), np.uint8), np.full((n, F), ord("N"), np.uint8)
    rnd_reads, rnd_refs = synth.make_pairs(n_random, R, F, seed=seed, **PAIR_ARGS)
    for k, p in enumerate(random_at):
        nul = np.nonzero(rnd_reads[k] == 0)[0]
        live = int(nul[0]) if nul.size else R            # (a read ends at its first NUL: what lies before it is rotated)
        reads[p] = rnd_reads[k]
        reads[p, :live] = np.roll(rnd_reads[k, :live], int(rng.integers(0, R)))
        refs[p] = rnd_refs[k]
        if k % 2 == 0:
            reads[p, rng.integers(1, R + 1):] = rng.choice([0, ord("N")])
    where = {}
    ties = _tie_rows(G, K, R, n_planted - 1)
    for i, p in enumerate(planted_at):
        c1 = (2 * i) % (F - 1)
        c2 = c1 + 1 + (3 * i) % (F - 1 - c1)
        if i == 0:
            c1, c2 = 0, F - 1                           # (row 0 / row R - 1 with column 0 / column F - 1)
        assert 0 <= c1 < c2 < F
        if i == n_planted - 1:                          # the tie in one row: the first column wins
            r = (R // 2 + K - 1) % R
            reads[p, r] = refs[p, c1] = refs[p, c2] = ord("A")
            where[p] = (r + 1, c1 + 1)
        else:
            r1, r2 = ties[i]
            reads[p, r1], reads[p, r2], refs[p, c1], refs[p, c2] = ord("A"), ord("C"), ord("C"), ord("A")
            where[p] = (r1 + 1, c2 + 1)
    reads.setflags(write=False)
    refs.setflags(write=False)
    return reads, refs, tuple(random_at), where


@functools.lru_cache(maxsize=None)
def reference(G, K, R, F, track, form):
    """placed_ref.placed of the case's batch under scoring_args(track, form, ...): int64 [n, 3], read-only"""
    reads, refs, _, _ = batch(G, K, R, F)
    exp = placed_ref.placed(reads, refs, _scoring(scoring_args(track, form, R, F, K)), affine=len(FORMS[form]) > 2)
    exp.setflags(write=False)
    return exp


def input_problems(G, K, R, F, track, form):
    """What the inputs of one run must be for the run to mean something, from the batch and the reference alone: at least half
    of the random pairs score; their end rows fall into at least two lanes of the register (R > K at every shape); at least one
    read is trimmed by more than K rows; the planted pairs' reference records are the construction's."""
    reads, refs, random_at, where = batch(G, K, R, F)
    exp = reference(G, K, R, F, track, form)
    match = scoring_args(track, form, R, F, K)[0]
    rnd = exp[list(random_at)]
    problems = []
    if 2 * (rnd[:, 0] > 0).sum() < len(rnd):
        problems.append(("fewer than half of the random pairs score", int((rnd[:, 0] > 0).sum()), len(rnd)))
    lanes = {int(r - 1 + G * K - R) // K for s, r, _ in rnd if s > 0}
    if R > K and len(lanes) < 2:
        problems.append(("the random pairs' end rows lie in one lane", sorted(lanes)))
    kept = [int(np.nonzero((reads[p] != 0) & (reads[p] != ord("N")))[0].max(initial=-1)) + 1 for p in random_at]
    if not any(R - k > K for k in kept):
        problems.append(("no read trimmed by more than K rows", kept))
    for p, (r, c) in where.items():
        if tuple(exp[p]) != (match, r, c):
            problems.append(("planted pair", p, "reference", exp[p].tolist(), "construction", (match, r, c)))
    return problems
