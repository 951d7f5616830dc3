"""Suboptimal Smith-Waterman scores on the GPU: 60 seeded random configurations -- shapes up to 160 x 300, the four gap forms,
random masks, planted and random pairs, ragged tails -- against tests/subopt_ref.py, exactly.

The oracle's own output is checked first, for EVERY configuration (oracle_checks): 52 of the 60 draw their mask from
{0, 1, R // 4, R // 2, R} and place the planted copy so that its window lies inside the reference; there at least half of the
planted pairs have score2 > 0, candidate columns exist on both sides of the window, and runner-ups are found on both.  The
other 8 (every seventh seed) take a mask of F or F + 5, which leaves no candidate at all: there score2 and ref_end2 are 0 on
every pair, and that is asserted instead -- neither condition can hold for them.  So no configuration compares zeros with
zeros unnoticed."""
import numpy as np
import pytest
import torch

import subopt_cases as cases
import subopt_ref
from versalignlib_amd import hipkernel

pytestmark = pytest.mark.gpu

FORMS = [(-3, -3), (-2, -4), (-3, -3, -5, -1, -5, -1), (-3, -3, -6, -2, -4, -1)]
SEEDS = 60


def _config(seed):
    """-> R, F, scoring, affine, mask, plant_at, candidates (False: the mask covers the whole reference)"""
    rng = np.random.default_rng(1000 + seed)
    R = int(rng.integers(8, 161))
    form = FORMS[seed % 4]
    match = int(rng.choice([1, 2, 3, 14, 60]))
    sc = hipkernel.Scoring.make(match, -int(rng.integers(1, match + 2)), *(g * (1 if match < 14 else match // 3) for g in form))
    if seed % 7 == 6:
        F = int(rng.integers(max(12, R // 2), 301))            # (references shorter than the read too)
        mask = F + int(rng.choice([0, 5]))
        plant_at = int(rng.integers(0, max(1, F - min(R, F) // 2)))
        return R, F, sc, len(form) > 2, mask, plant_at, False
    # the planted copy ends in column plant_at + R - 1; columns 0 .. plant_at + R - 2 - mask lie left of its window and
    # plant_at + R + mask .. F - 1 right of it: with plant_at >= 2 and plant_at + R + mask + 2 <= F neither side is empty
    mask = int(rng.choice([m for m in (0, 1, R // 4, R // 2, R) if R + m + 4 <= 300]))
    F = int(rng.integers(R + mask + 4, 301))
    plant_at = int(rng.integers(2, F - R - mask - 1))
    return R, F, sc, len(form) > 2, mask, plant_at, True


def oracle_checks(exp, refs, planted_rows, mask, candidates):
    """what the issue asks of every planted batch, on the oracle's records"""
    if not candidates:
        assert (exp[:, 3:] == 0).all()
        return
    assert 2 * int((exp[planted_rows, 3] > 0).sum()) >= int(planted_rows.sum()), (int((exp[planted_rows, 3] > 0).sum()), int(planted_rows.sum()))
    end, Fp, scored = exp[:, 2] - 1, subopt_ref.trimmed_lengths(refs), exp[:, 0] > 0
    has_left, has_right = scored & (end - mask - 1 >= 0), scored & (end + mask + 1 <= Fp - 1)
    assert has_left[planted_rows].any() and has_right[planted_rows].any(), (int(has_left.sum()), int(has_right.sum()))
    hit = exp[:, 3] > 0
    assert (np.abs(exp[hit, 4] - exp[hit, 2]) > mask).all()
    left, right = int((exp[hit, 4] < exp[hit, 2]).sum()), int((exp[hit, 4] > exp[hit, 2]).sum())
    assert left > 0 and right > 0, (left, right)          # ... and the runner-up itself is found on either side within the batch


def test_the_configurations():
    configs = [_config(seed) for seed in range(SEEDS)]
    assert sum(not c[6] for c in configs) == 8 and {c[3] for c in configs if not c[6]} == {False, True}
    assert max(c[0] for c in configs) > 128 and max(c[1] for c in configs) > 256 and all(c[0] <= 160 and c[1] <= 300 for c in configs)
    for R, F, _, _, mask, plant_at, candidates in configs:
        assert not candidates or (plant_at >= 2 and plant_at + R + mask + 2 <= F)
        assert candidates or mask >= F
    for drawn in (lambda R: 0, lambda R: 1, lambda R: R // 4, lambda R: R // 2, lambda R: R):          # every kind of mask is drawn
        assert any(c[6] and c[0] >= 8 and c[4] == drawn(c[0]) for c in configs)


@pytest.mark.parametrize("block", range(6))
def test_fuzz(block):
    for seed in range(10 * block, 10 * block + 10):
        R, F, sc, affine, mask, plant_at, candidates = _config(seed)
        n = 24 + seed % 9
        reads, refs, planted_rows = cases.fuzz_batch(n, R, F, seed=seed, plant_at=plant_at)
        exp = subopt_ref.subopt(reads, refs, sc, mask, affine=affine, chunk=64)
        oracle_checks(exp, refs, planted_rows, mask, candidates)
        eng = hipkernel.Engine(R, F, sc)
        out = eng.score_subopt_device(0, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda(), mask)
        torch.cuda.synchronize()
        got = out.cpu().numpy().astype(np.int64)
        ran = eng.describe(0, n)["ran_subopt"]
        eng.close()
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, (seed, R, F, mask, ran, bad[:8].tolist(), got[bad[:4]].tolist(), exp[bad[:4]].tolist())
        assert ran in ("key", "rows")


def test_the_planted_generator_has_runner_ups_on_both_sides():
    # the issue's generator: R = 33, F = 70, mask = 16, half of the reads planted at column 10
    R, F, mask = 33, 70, 16
    sc = hipkernel.Scoring.make(2, -1, -3, -3)
    reads, refs, planted = cases.fuzz_batch(64, R, F, seed=99, plant_at=10)
    exp = subopt_ref.subopt(reads, refs, sc, mask)
    oracle_checks(exp, refs, planted, mask, True)
    eng = hipkernel.Engine(R, F, sc)
    out = eng.score_subopt_device(0, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda(), mask)
    torch.cuda.synchronize()
    eng.close()
    assert np.array_equal(out.cpu().numpy().astype(np.int64), exp)
