"""Seeded differential sweep of the banded NW variant (band_nw = 1): shapes, bands and scoring parameters no hand-written case
names -- zero and equal gap scores, reads longer than the reference, bands of a few diagonals, every affine variant -- scores
and alignments of libHIPKernel.so against band_nw_ref.py on the block band describe() reports, bit-exact.  Bands whose windows
do not connect must be refused.  Deterministic: the configurations come from the case number."""
import numpy as np
import pytest

from oracle import cpu_ref
from versalignlib_amd import build, hipkernel, host, synth
import band_nw_ref as bnr

pytestmark = pytest.mark.gpu
CASES = 48


def _draw(case):
    rng = np.random.default_rng(7700 + case)
    kind = case % 4
    if kind == 0:
        R, F = int(rng.integers(8, 120)), int(rng.integers(8, 200))
    elif kind == 1:
        R, F = int(rng.integers(100, 500)), int(rng.integers(200, 900))
    elif kind == 2:
        R, F = int(rng.integers(300, 900)), int(rng.integers(40, 300))          # read longer than ref
    else:
        R, F = int(rng.integers(600, 1500)), int(rng.integers(600, 1500))
    band = int(rng.choice([2, 3, 4, 8, 16, 33, 64, 200]))
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
    return dict(R=R, F=F, band=band, match=match, mismatch=mismatch, gap_read=gap_read, gap_ref=gap_ref, affine=affine, seed=case)


@pytest.mark.parametrize("case", range(CASES))
def test_case(case):
    c = _draw(case)
    R, F, band = c["R"], c["F"], c["band"]
    reads, refs = synth.make_pairs(6, R, F, seed=300 + c["seed"], sub_rate=0.1, indel_rate=0.02, n_run_frac=0.2, short_frac=0.2, junk_frac=0.1)
    params = dict(score_match=c["match"], score_mismatch=c["mismatch"], score_gap_read=c["gap_read"], score_gap_ref=c["gap_ref"],
                  band_width=band, band_alignments=1, band_nw=1, num_threads=2)
    args = [c["match"], c["mismatch"], c["gap_read"], c["gap_ref"]]
    if c["affine"]:
        params.update(zip(("score_gap_open_read", "score_gap_extend_read", "score_gap_open_ref", "score_gap_extend_ref"), c["affine"]))
        args += list(c["affine"])
    sc = cpu_ref.Scoring.make(*args)
    connects = 2 * (band // 2) + 1 >= -(-F // R)
    with host.Plugin(build.HIP_PLUGIN, R, F, **params) as hip:
        if not connects:
            with pytest.raises(host.PluginError, match="do not connect"):
                hip.score_alignments(1, reads, refs)
            with pytest.raises(host.PluginError, match="do not connect"):
                hip.compute_alignments(1, reads, refs)
            return
        scores = hip.score_alignments(1, reads, refs)
        rows, idx = hip.compute_alignments(1, reads, refs)
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*args))
    eng.set_band_width(band)
    eng.set_band_nw(1)
    d = eng.describe(1, 6)
    eng.close()
    shape = (d["band_block_rows"], d["band_col_align"])
    exp_scores = bnr.score_banded_nw(reads, refs, band, sc, *shape, affine=bool(c["affine"]))
    assert np.array_equal(scores.astype(np.int64), np.minimum(exp_scores, 32767)), (c, shape)
    exp_rows, exp_idx = bnr.align_banded_nw(reads, refs, band, sc, *shape, affine=bool(c["affine"]))
    bad = [p for p in range(6) if not (np.array_equal(rows[p], exp_rows[p]) and np.array_equal(idx[p], exp_idx[p]))]
    assert not bad, (c, shape, bad, idx[bad[0]], exp_idx[bad[0]])
