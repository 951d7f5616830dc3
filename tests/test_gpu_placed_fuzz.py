"""Seeded differential sweep of the placed Smith-Waterman scores: shapes and scoring parameters no hand-written case names --
zero and equal gap scores, reads longer than the reference, every affine variant -- against tests/placed_ref.py, bit-exact,
through the device and the host entry point.  About one case in six asks for something the rule refuses (the NW variant, a band,
traceback_policy = 1, int32 cells): those must be refused.  Deterministic: the configurations come from the case number."""
import numpy as np
import pytest
import torch

import placed_ref
from versalignlib_amd import hipkernel, synth

pytestmark = pytest.mark.gpu
CASES = 48
SEED = 9124


def _draw(case):
    rng = np.random.default_rng(SEED + case)
    R, F = int(rng.integers(8, 401)), int(rng.integers(8, 701))
    match, mismatch = int(rng.integers(0, 7)), -int(rng.integers(0, 6))
    gap_read, gap_ref = -int(rng.integers(0, 8)), -int(rng.integers(0, 8))
    if rng.random() < 0.3:
        gap_ref = gap_read
    affine = None
    if rng.random() < 0.5:
        o_r, o_f = -int(rng.integers(0, 10)), -int(rng.integers(0, 10))
        if rng.random() < 0.4:
            o_f = o_r
        affine = (o_r, max(-int(rng.integers(0, 5)), o_r), o_f, max(-int(rng.integers(0, 5)), o_f))
        if o_f == o_r and rng.random() < 0.5:
            affine = (o_r, affine[1], o_r, affine[1])
    refusal = str(rng.choice(["nw", "band", "policy", "width"])) if rng.random() < 0.17 else None
    return dict(R=R, F=F, match=match, mismatch=mismatch, gap_read=gap_read, gap_ref=gap_ref, affine=affine, refusal=refusal, seed=case)


def _refused_by_the_rule(c):
    """the reference statement of the rule's refusals: the four modes, or cells that could leave int16"""
    top = min(c["R"], c["F"]) * max(c["match"], 0) + 1
    low = min(c["mismatch"], 0) + min([c["gap_read"], c["gap_ref"], 0] + list(c["affine"] or ()))
    return c["refusal"] is not None or top > 32000 or low < -32000


def test_the_seed_keeps_refusals_to_a_quarter():
    refused = [case for case in range(CASES) if _refused_by_the_rule(_draw(case))]
    assert 0 < len(refused) <= CASES // 4, refused


@pytest.mark.parametrize("case", range(CASES))
def test_case(case):
    assert sum(_refused_by_the_rule(_draw(k)) for k in range(CASES)) <= CASES // 4          # (CPU side, before any GPU call)
    c = _draw(case)
    R, F = c["R"], c["F"]
    reads, refs = synth.make_pairs(32, R, F, seed=500 + c["seed"], sub_rate=0.1, indel_rate=0.02, n_run_frac=0.2, short_frac=0.2, junk_frac=0.1)
    args = [c["match"], c["mismatch"], c["gap_read"], c["gap_ref"]] + list(c["affine"] or ())
    sc = hipkernel.Scoring.make(*args)
    eng = hipkernel.Engine(R, F, sc)
    opt = 0
    if c["refusal"] == "nw":
        opt = 1
    elif c["refusal"] == "band":
        eng.set_band_width(int(8 + case))
    elif c["refusal"] == "policy":
        eng.set_traceback_policy(1)
    elif c["refusal"] == "width":
        eng.set_score_width(32)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    if _refused_by_the_rule(c):
        with pytest.raises(hipkernel.HipKernelError):
            eng.score_placed_device(opt, d_reads, d_refs)
        with pytest.raises(hipkernel.HipKernelError):
            eng.score_placed_host(opt, reads, refs)
        assert eng.describe(0, 32)["ran_placed"] == "none"
        eng.close()
        return
    got = eng.score_placed_device(opt, d_reads, d_refs)
    torch.cuda.synchronize()
    got = got.cpu().numpy().astype(np.int64)
    ran = eng.describe(0, 32)["ran_placed"]
    host = eng.score_placed_host(opt, reads, refs, threads=2)
    eng.close()
    exp = placed_ref.placed(reads, refs, sc, affine=c["affine"] is not None)
    assert ran in ("key", "rows"), ran
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (c, ran, bad[:6].tolist(), got[bad[:3]].tolist(), exp[bad[:3]].tolist())
    assert np.array_equal(np.stack([host["score"], host["read_end"], host["ref_end"]], axis=1).astype(np.int64), exp), (c, "host path")
