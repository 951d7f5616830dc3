"""Banded Smith-Waterman alignments (band_alignments = 1): the strips of align_strip_kernel<..., BAND> and
traceback_band_kernel against the numpy restatement of band_align_ref.py, on the block band describe() reports."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from versalignlib_amd import build, hipkernel, host, synth
from conftest import debug_switches
import band_align_ref as bar
from test_band_align_ref import shifted_insertion_pairs

pytestmark = pytest.mark.gpu

LINEAR = (2, -1, -3, -2)
AFFINE = (2, -1, -3, -3, -5, -1, -4, -2)
PLUGIN_AFFINE = dict(score_gap_open_read=-5, score_gap_extend_read=-1, score_gap_open_ref=-4, score_gap_extend_ref=-2)


def _pairs(n, R, F, seed):
    return synth.make_pairs(n, R, F, seed=seed, sub_rate=0.1, indel_rate=0.01, n_run_frac=0.2, short_frac=0.15,
                            lowercase_frac=0.05, junk_frac=0.05)


def _plugin(R, F, band, affine, match=2, **extra):
    params = dict(score_match=match, score_mismatch=-1, score_gap_read=-3, score_gap_ref=-2 if not affine else -3,
                  band_width=band, band_alignments=1, num_threads=4)
    if affine:
        params.update(PLUGIN_AFFINE)
    params.update(extra)
    return host.Plugin(build.HIP_PLUGIN, R, F, **params)


def _scoring(affine, match=2):
    return cpu_ref.Scoring.make(match, -1, -3, -3, -5, -1, -4, -2) if affine else cpu_ref.Scoring.make(match, -1, -3, -2)


def _check_plugin(reads, refs, band, affine, expect_fill=None, match=2):
    R, F = reads.shape[1], refs.shape[1]
    sc = _scoring(affine, match)
    with _plugin(R, F, band, affine, match) as hip:
        rows, idx = hip.compute_alignments(0, reads, refs)
        ran = hip.last_ran()
        scores = hip.score_alignments(0, reads, refs)
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*((match,) + (AFFINE if affine else LINEAR)[1:])))
    eng.set_band_width(band)
    d = eng.describe(0, len(reads))
    eng.close()
    block_rows, col_align = d["band_block_rows"], d["band_col_align"]
    exp_rows, exp_idx = bar.align_banded_sw(reads, refs, band, sc, block_rows, col_align, affine=affine)
    bad = [p for p in range(len(reads)) if not (np.array_equal(rows[p], exp_rows[p]) and np.array_equal(idx[p], exp_idx[p]))]
    assert not bad, (block_rows, col_align, bad[:8], idx[bad[0]], exp_idx[bad[0]])
    # per pair, the rescored alignment is the banded score (where the score's int16 did not saturate)
    fits = scores < 32767
    assert np.array_equal(bar.rescore(rows, idx, sc, affine)[fits], scores[fits].astype(np.int64))
    if expect_fill:
        assert ran["ran_align_fill"] == expect_fill, ran
    return block_rows, col_align


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("R,F,n,band,seed", [(150, 500, 24, 32, 1), (3000, 2800, 6, 64, 2), (3000, 2800, 6, 512, 3)])
def test_banded_alignments_match_the_restatement(affine, R, F, n, band, seed):
    reads, refs = _pairs(n, R, F, seed)
    _check_plugin(reads, refs, band, affine, expect_fill="strip_band")


@pytest.mark.parametrize("affine", [False, True])
def test_shifted_insertions(affine):
    reads, refs = shifted_insertion_pairs(n=12)
    _check_plugin(reads, refs, 64, affine, expect_fill="strip_band")


@pytest.mark.parametrize("affine", [False, True])
def test_strip_band_blocks_under_no_band_chain(affine, monkeypatch):
    debug_switches(monkeypatch, no_band_chain=1)
    reads, refs = shifted_insertion_pairs(n=8, seed=4)
    assert _check_plugin(reads, refs, 64, affine, expect_fill="strip_band") == (160, 4)


@pytest.mark.parametrize("affine", [False, True])
def test_wide_band_is_the_unbanded_oracle(affine):
    R, F = 700, 900
    reads, refs = _pairs(16, R, F, 5)
    sc = _scoring(affine)
    with _plugin(R, F, 2 * max(R, F), affine) as hip:
        rows, idx = hip.compute_alignments(0, reads, refs)
    exp_rows, exp_idx = cpu_ref.align(0, reads, refs, sc, threads=4, affine=affine, wide=True)
    assert np.array_equal(idx, exp_idx) and np.array_equal(rows, exp_rows)


@pytest.mark.parametrize("affine", [False, True])
def test_int32_cells(affine):
    """match 20 on 2,000-base reads: cells leave int16, the banded strips run on int32 cells."""
    reads, refs = synth.make_pairs(4, 2000, 2000, seed=6, sub_rate=0.02, indel_rate=0.002)
    _check_plugin(reads, refs, 128, affine, expect_fill="strip_wide_band", match=20)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_small_calls_and_device_entry_point(n):
    R, F, band = 150, 500, 16
    reads, refs = _pairs(n, R, F, 20 + n)
    exp_rows, exp_idx = bar.align_banded_sw(reads, refs, band, _scoring(False), *_shape(R, F, band))
    with _plugin(R, F, band, False) as hip:
        rows, idx = hip.compute_alignments(0, reads, refs)
        assert hip.last_ran()["ran_align_fill"] == "strip_band"
    assert np.array_equal(idx, exp_idx) and np.array_equal(rows, exp_rows)
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*LINEAR))
    eng.set_band_width(band)
    eng.set_band_alignments(1)
    d_rows, d_idx = eng.align_device(0, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda())
    torch.cuda.synchronize()
    assert eng.describe(0, n)["ran_align_fill"] == "strip_band"
    eng.close()
    assert np.array_equal(d_idx.cpu().numpy(), exp_idx) and np.array_equal(d_rows.cpu().numpy(), exp_rows)


def _shape(R, F, band):
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*LINEAR))
    eng.set_band_width(band)
    d = eng.describe(0, 1)
    eng.close()
    return d["band_block_rows"], d["band_col_align"]


def test_shards_honour_the_key():
    R, F, band = 1200, 1200, 64
    reads, refs = shifted_insertion_pairs(n=9, seed=7)
    exp_rows, exp_idx = bar.align_banded_sw(reads, refs, band, _scoring(False), *_shape(R, F, band))
    with _plugin(R, F, band, False, hip_devices=3) as hip:
        rows, idx = hip.compute_alignments(0, reads, refs)
    assert np.array_equal(idx, exp_idx) and np.array_equal(rows, exp_rows)


def test_refusals():
    R, F = 300, 300
    reads, refs = _pairs(4, R, F, 8)
    with _plugin(R, F, 32, False) as hip:
        with pytest.raises(host.PluginError, match="Smith-Waterman alignments only"):
            hip.compute_alignments(1, reads, refs)
    with _plugin(R, F, 32, False, traceback_policy=1) as hip:
        with pytest.raises(host.PluginError, match="traceback_policy"):
            hip.compute_alignments(0, reads, refs)
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*LINEAR))
    with pytest.raises(hipkernel.HipKernelError, match="band_alignments must be 0 or 1"):
        eng.set_band_alignments(2)
    eng.close()


@pytest.mark.parametrize("affine", [False, True])
def test_key_off_keeps_unbanded_alignments(affine):
    R, F = 1200, 1200
    reads, refs = shifted_insertion_pairs(n=8, seed=11)
    sc = _scoring(affine)
    with _plugin(R, F, 64, affine, band_alignments=0) as hip:
        rows, idx = hip.compute_alignments(0, reads, refs)
    exp_rows, exp_idx = cpu_ref.align(0, reads, refs, sc, threads=4, affine=affine, wide=True)
    assert np.array_equal(idx, exp_idx) and np.array_equal(rows, exp_rows)


def test_pointer_stream_shrinks_with_the_band():
    """align_ptr_bytes_per_pair of the plan at 10 kbp x 10 kbp, band 512: at most 1/5 of the unbanded plan's (two pairs each)."""
    R = F = 10000
    reads, refs = synth.make_pairs(2, R, F, seed=12, sub_rate=0.05)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    per_pair = {}
    for on in (0, 1):
        eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*LINEAR))
        eng.set_band_width(512)
        eng.set_band_alignments(on)
        eng.align_device(0, d_reads, d_refs)
        torch.cuda.synchronize()
        d = eng.describe(0, 2)
        assert d["band_alignments"] == on
        per_pair[on] = d["align_ptr_bytes_per_pair"]
        eng.close()
    assert 0 < per_pair[1] * 5 <= per_pair[0], per_pair
