"""Extension scores on the GPU: 48 seeded random configurations -- shapes up to 200 x 300, the four gap forms at several scales,
the engine's own geometry or a forced one (full geometries, and others, which are re-planned onto the next full one), planted
extensions with gaps and mismatches, ragged tails, interior junk -- against tests/extend_ref.py, exactly.

The oracle's own output is checked first, for every configuration: some pairs extend (score > 0, with an end cell inside the
trimmed lengths), some do not (five values with score 0), read-end scores come out negative as well as positive, and at least
one read-end score sits in the border column or ends before the trimmed reference does.  So no configuration compares zeros with
zeros unnoticed."""
import numpy as np
import pytest
import torch

import extend_ref
import instance_matrix as im
from versalignlib_amd import hipkernel

pytestmark = pytest.mark.gpu

FORMS = [(-3, -3), (-2, -4), (-3, -3, -5, -1, -5, -1), (-3, -3, -6, -2, -4, -1)]
SEEDS = 48
BASES = np.frombuffer(b"ACGT", np.uint8)
SCALE = {1: 1, 2: 1, 3: 1, 14: 4, 60: 10}           # gap scale by match: 500 steps at 60 and the largest addend stay above -32000


def _config(seed):
    """-> R, F, scoring, affine, G, K (0, 0: the engine's own geometry)"""
    rng = np.random.default_rng(2000 + seed)
    R, F = int(rng.integers(1, 201)), int(rng.integers(1, 301))
    form = FORMS[seed % 4]
    match = int(rng.choice([1, 2, 3, 14, 60]))
    sc = hipkernel.Scoring.make(match, -int(rng.integers(1, match + 2)), *(g * SCALE[match] for g in form))
    G, K = 0, 0
    if seed % 3:
        fits = [gk for gk in sorted(im.GEOMETRIES) if gk[0] * gk[1] >= R and (seed % 3 == 1) == im.GEOMETRIES[gk]]
        G, K = fits[int(rng.integers(0, len(fits)))]
    return R, F, sc, len(form) > 2, G, K


def _batch(n, R, F, seed):
    rng = np.random.default_rng(seed)
    reads, refs = BASES[rng.integers(0, 4, (n, R))], BASES[rng.integers(0, 4, (n, F))]
    for p in range(n):
        if p % 3 < 2:                                   # an extension from the anchor, two thirds of the pairs
            L = int(rng.integers(1, min(R, F) + 1))
            shift = int(rng.integers(0, 3)) if p % 3 == 1 else 0          # ... a third behind 0-2 extra reference bases
            span = min(L, F - shift)
            if span > 0:
                refs[p, shift:shift + span] = reads[p, :span]
            if span > 6 and rng.random() < 0.5:
                refs[p, shift + span // 2] = BASES[(int(np.searchsorted(BASES, refs[p, shift + span // 2])) + 1) % 4]
        if rng.random() < 0.3:
            reads[p, int(rng.integers(0, R + 1)):] = rng.choice([0, ord("N")])
        if rng.random() < 0.3:
            refs[p, int(rng.integers(0, F + 1)):] = rng.choice([0, ord("N")])
        if rng.random() < 0.2:
            reads[p, int(rng.integers(0, R))] = rng.choice([0, ord("N"), 0x80, 0xFF])
        if rng.random() < 0.2:
            refs[p, int(rng.integers(0, F))] = rng.choice([0, ord("N"), 0x80, 0xFF])
    reads[n - 1], refs[n - 1] = BASES[rng.integers(0, 4, R)], ord("N")          # a read against no reference: the border column wins
    return reads, refs


def oracle_checks(exp, reads, refs):
    Rp, Fp = extend_ref.trimmed_lengths(reads), extend_ref.trimmed_lengths(refs)
    hit = exp[:, 0] > 0
    assert (exp[~hit, :3] == 0).all() and (exp[hit, 1] >= 1).all() and (exp[hit, 1] <= Rp[hit]).all() and (exp[hit, 2] <= Fp[hit]).all()
    assert (exp[Rp == 0] == 0).all() and (exp[:, 4] >= 0).all() and (exp[:, 4] <= Fp).all()
    assert (exp[Fp > 0, 3] <= exp[Fp > 0, 0]).all()


def test_the_configurations():
    configs = [_config(seed) for seed in range(SEEDS)]
    assert max(c[0] for c in configs) > 160 and max(c[1] for c in configs) > 256 and min(c[0] for c in configs) < 16
    assert all(1 <= c[0] <= 200 and 1 <= c[1] <= 300 for c in configs)
    assert {c[3] for c in configs} == {False, True}
    forced = [(c[4], c[5]) for c in configs if c[4]]
    assert len(forced) == 32 and any(im.GEOMETRIES[gk] for gk in forced) and any(not im.GEOMETRIES[gk] for gk in forced)
    assert sum(1 for c in configs if not c[4]) == 16


@pytest.mark.parametrize("block", range(6))
def test_fuzz(block):
    seen_hit = seen_empty = seen_negative = seen_border = 0
    for seed in range(8 * block, 8 * block + 8):
        R, F, sc, affine, G, K = _config(seed)
        n = 24 + seed % 9
        reads, refs = _batch(n, R, F, seed)
        exp = extend_ref.extend(reads, refs, sc, affine=affine, chunk=64)
        oracle_checks(exp, reads, refs)
        seen_hit += int((exp[:, 0] > 0).sum())
        seen_empty += int((exp[:, 0] == 0).sum())
        seen_negative += int((exp[:, 3] < 0).sum())
        seen_border += int(((exp[:, 4] == 0) & (extend_ref.trimmed_lengths(reads) > 0)).sum())
        eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
        out = eng.score_extend_device(0, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda())
        torch.cuda.synchronize()
        got = out.cpu().numpy().astype(np.int64)
        ran = eng.describe(0, n)["ran_extend"]
        eng.close()
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, (seed, R, F, G, K, affine, bad[:8].tolist(), got[bad[:4]].tolist(), exp[bad[:4]].tolist())
        assert ran == "rows"
    assert seen_hit > 0 and seen_empty > 0 and seen_negative > 0 and seen_border > 0, (seen_hit, seen_empty, seen_negative, seen_border)
