"""Seeded differential sweep of the spanned Smith-Waterman scores: shapes and scoring parameters no hand-written case names --
zero and equal gap scores (the reverse sweep then runs unclipped), match 0, reads longer than the reference, every affine
variant, a forced full geometry in a third of the cases -- against tests/span_ref.py, bit-exact, through the device or the host
entry point (the case number decides which; the other one is compared with it).  About one case in six asks for something the
rule refuses (the NW variant, a band with or without band_placed, traceback_policy = 1, int32 cells): those must be refused.
Deterministic: the configurations come from the case number."""
import numpy as np
import pytest
import torch

import span_cases as sc_
import span_ref
from versalignlib_amd import hipkernel, synth

pytestmark = pytest.mark.gpu
CASES = 48
SEED = 7311
FULL = [(8, 8), (16, 10), (32, 10), (64, 8)]


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
    refusal = str(rng.choice(["nw", "band", "band_placed", "policy", "width"])) if rng.random() < 0.17 else None
    forced = next(g for g in FULL if g[0] * g[1] >= R) if rng.random() < 0.33 else (0, 0)
    entry = "host" if case % 3 == 2 else "device"
    return dict(R=R, F=F, match=match, mismatch=mismatch, gap_read=gap_read, gap_ref=gap_ref, affine=affine, refusal=refusal, forced=forced,
                entry=entry, seed=case)


def test_the_seed_keeps_refusals_to_a_quarter_and_covers_the_edges():
    draws = [_draw(case) for case in range(CASES)]
    refused = [c for c in draws if c["refusal"] is not None]
    assert 0 < len(refused) <= CASES // 4, len(refused)
    assert any(c["forced"] != (0, 0) for c in draws) and any(c["affine"] for c in draws) and any(c["R"] > c["F"] for c in draws)
    scs = [hipkernel.Scoring.make(*([c["match"], c["mismatch"], c["gap_read"], c["gap_ref"]] + list(c["affine"] or ()))) for c in draws]
    clipped = [sc_.span_ref_length(c["R"], c["F"], sc) < c["F"] for c, sc in zip(draws, scs)]
    assert any(clipped) and not all(clipped)


@pytest.mark.parametrize("case", range(CASES))
def test_case(case):
    c = _draw(case)
    R, F = c["R"], c["F"]
    reads, refs = synth.make_pairs(32, R, F, seed=900 + c["seed"], sub_rate=0.1, indel_rate=0.02, n_run_frac=0.2, short_frac=0.2, junk_frac=0.1)
    args = [c["match"], c["mismatch"], c["gap_read"], c["gap_ref"]] + list(c["affine"] or ())
    sc = hipkernel.Scoring.make(*args)
    eng = hipkernel.Engine(R, F, sc, group_lanes=c["forced"][0], rows_per_lane=c["forced"][1])
    opt = 0
    if c["refusal"] == "nw":
        opt = 1
    elif c["refusal"] in ("band", "band_placed"):
        eng.set_band_width(int(8 + case))
        eng.set_band_placed(1 if c["refusal"] == "band_placed" else 0)
    elif c["refusal"] == "policy":
        eng.set_traceback_policy(1)
    elif c["refusal"] == "width":
        eng.set_score_width(32)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    if c["refusal"] is not None:
        with pytest.raises(hipkernel.HipKernelError):
            eng.score_span_device(opt, d_reads, d_refs)
        with pytest.raises(hipkernel.HipKernelError):
            eng.score_span_host(opt, reads, refs)
        assert eng.describe(0, 32)["ran_span"] == "none"
        eng.close()
        return
    dev = eng.score_span_device(opt, d_reads, d_refs)
    torch.cuda.synchronize()
    dev = dev.cpu().numpy().astype(np.int64)
    d = eng.describe(0, 32)
    host = eng.score_span_host(opt, reads, refs, threads=2)
    eng.close()
    host = np.stack([host[k] for k in hipkernel.span_dtype().names], axis=1).astype(np.int64)
    exp = span_ref.spans(reads, refs, sc, affine=c["affine"] is not None)
    assert d["span_ref_length"] == sc_.span_ref_length(R, F, sc), (c, d["span_ref_length"])
    assert all(part in ("key", "rows") for part in d["ran_span"].split("/")) and d["ran_span"].count("/") == 1, d["ran_span"]
    got, other = (host, dev) if c["entry"] == "host" else (dev, host)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (c, d["ran_span"], bad[:6].tolist(), got[bad[:3]].tolist(), exp[bad[:3]].tolist())
    assert np.array_equal(other, got), (c, "the other entry point")
