"""Inputs the CPU and the GPU tests of the spanned scores share: the gap forms and pair settings of tests/test_gpu_placed.py, and
batches built by hand whose begin cell the construction states, independently of any fill."""
import numpy as np

from versalignlib_amd import hipkernel, synth

# linear symmetric, linear gap_read != gap_ref, affine symmetric, affine with four scores
FORMS = {"sym": (-3, -3), "lin": (-2, -4), "affsym": (-3, -3, -5, -1, -5, -1), "aff": (-3, -3, -6, -2, -4, -1)}
SHAPES = [(12, 20), (33, 70), (40, 9), (20, 120)]


def scoring(form, match=2, mismatch=-1):
    return hipkernel.Scoring.make(match, mismatch, *FORMS[form])


def is_affine(form):
    return len(FORMS[form]) > 2


def pairs(n, R, F, seed, **kw):
    args = dict(sub_rate=0.1, indel_rate=0.02, n_run_frac=0.1, short_frac=0.1, lowercase_frac=0.05, junk_frac=0.04)
    args.update(kw)
    return synth.make_pairs(n, R, F, seed=seed, **args)


def span_ref_length(R, F, sc):
    """the bound of cell_rules.h, restated: min(F, R + (R m - 1) // c)"""
    m = max(sc.match, sc.mismatch, 0)
    c = min(abs(sc.open_read), abs(sc.ext_read)) if sc.affine else abs(sc.gap_read)
    if c == 0:
        return F
    return min(F, R + ((R * m - 1) // c if R * m >= 1 else 0))


def tie_scoring(form):
    """2 / -2: one match and one mismatch net exactly 0; gaps dear enough that no path leaves a motif's diagonal"""
    return hipkernel.Scoring.make(2, -2, -7, -7) if form == "sym" else hipkernel.Scoring.make(2, -2, -7, -7, -9, -7, -8, -7)


def _motif(p, m):
    """m bases without a repeat at any shift (no chance alignment beside the motif's own diagonal), rotated with p"""
    base = np.frombuffer(b"ACGTAGCTGACT", np.uint8)
    return np.roll(base, -(p % 4))[:m].copy()


def _other(base):
    return np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), base)]


def tie_batches(R, F, n=16):
    """name -> (reads, refs, expected int64 [n, 5]) under tie_scoring: everything is N but what is written here.
    zero_block: a motif preceded, on its diagonal, by one match and then one mismatch (+2 - 2 = 0): two optimal alignments end
                in the end cell, the spanned record begins at the motif (the LATER begin);
    n_columns:  a motif preceded on its diagonal by N against N (score 0 each): every alignment that starts in the Ns and runs
                into the motif ties with the motif's own; the record begins at the motif, not in the Ns."""
    out = {}
    reads = np.full((n, R), ord("N"), np.uint8)
    refs = np.full((n, F), ord("N"), np.uint8)
    exp = np.zeros((n, 5), np.int64)
    for p in range(n):
        m = 4 + p % 4
        r0 = 2 + p % max(1, R - m - 2)
        c0 = 2 + (3 * p) % max(1, F - m - 2)
        r0, c0 = min(r0, R - m), min(c0, F - m)
        a = _motif(p, m)
        reads[p, r0:r0 + m] = a
        refs[p, c0:c0 + m] = a
        x = _other(_other(a[0]))
        reads[p, r0 - 2] = refs[p, c0 - 2] = x                 # a match ...
        reads[p, r0 - 1] = a[0]
        refs[p, c0 - 1] = _other(a[0])                         # ... then a mismatch: the block nets 0
        # (a[0] before the motif in the read: it cannot extend the motif, the reference holds another base there)
        exp[p] = (2 * m, r0, r0 + m, c0, c0 + m)
    out["zero_block"] = (reads, refs, exp)
    reads = np.full((n, R), ord("N"), np.uint8)
    refs = np.full((n, F), ord("N"), np.uint8)
    exp = np.zeros((n, 5), np.int64)
    for p in range(n):
        m = 4 + p % 4
        r0 = min(3 + p % max(1, R - m - 3), R - m)
        c0 = min(3 + (5 * p) % max(1, F - m - 3), F - m)
        a = _motif(p, m)
        reads[p, r0:r0 + m] = a
        refs[p, c0:c0 + m] = a
        exp[p] = (2 * m, r0, r0 + m, c0, c0 + m)
    out["n_columns"] = (reads, refs, exp)
    return out


def border_batch(R, F):
    """End cell and begin cell in row 0 / column 0 / the last row / the last column: motifs of one base or of a full diagonal,
    everything else N.  -> (reads, refs, expected [n, 5]) under any scoring with match 2 and negative mismatch / gaps"""
    d = min(R, F)
    spots = [(0, 0, 1), (0, F - 1, 1), (R - 1, 0, 1), (R - 1, F - 1, 1), (0, 0, d), (R - d, F - d, d), (0, F - d, d), (R - d, 0, d),
             (0, F // 2, 1), (R // 2, 0, 1), (R - 1, F // 2, 1), (R // 2, F - 1, 1)]
    n = len(spots)
    reads = np.full((n, R), ord("N"), np.uint8)
    refs = np.full((n, F), ord("N"), np.uint8)
    exp = np.zeros((n, 5), np.int64)
    motif = np.frombuffer((b"ACGTTGCAAGTC" * (d // 12 + 1))[:d], np.uint8)
    for p, (r, c, m) in enumerate(spots):
        reads[p, r:r + m] = motif[:m]
        refs[p, c:c + m] = motif[:m]
        exp[p] = (2 * m, r, r + m, c, c + m)
    return reads, refs, exp
