"""The banded NW variant (band_nw = 1) on the GPU: scores on the cyclic block chain (score_band_kernel<..., NW>) or the banded
strips (score_long_kernel<..., NWBAND>), alignments on the banded strips (align_strip_kernel / align_strip_wide_kernel
<K, kAlgNW, ..., BAND>) with traceback_band_kernel, against the numpy restatement of band_nw_ref.py on the block band
describe() reports -- through the plugin ABI and the flat device API."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from versalignlib_amd import build, hipkernel, host, synth
from conftest import debug_switches
import band_nw_ref as bnr
import cigar_ref
from test_band_align_ref import shifted_insertion_pairs

pytestmark = pytest.mark.gpu

LINEAR = (2, -1, -3, -2)
AFFINE = (2, -1, -3, -3, -5, -1, -4, -2)
PLUGIN_AFFINE = dict(score_gap_open_read=-5, score_gap_extend_read=-1, score_gap_open_ref=-4, score_gap_extend_ref=-2)
NW = 1


def _pairs(n, R, F, seed):
    return synth.make_pairs(n, R, F, seed=seed, sub_rate=0.1, indel_rate=0.01, n_run_frac=0.2, short_frac=0.15,
                            lowercase_frac=0.05, junk_frac=0.05)


def _plugin(R, F, band, affine, match=2, **extra):
    params = dict(score_match=match, score_mismatch=-1, score_gap_read=-3, score_gap_ref=-2 if not affine else -3,
                  band_width=band, band_alignments=1, band_nw=1, num_threads=4)
    if affine:
        params.update(PLUGIN_AFFINE)
    params.update(extra)
    return host.Plugin(build.HIP_PLUGIN, R, F, **params)


def _scoring(affine, match=2):
    return cpu_ref.Scoring.make(match, -1, -3, -3, -5, -1, -4, -2) if affine else cpu_ref.Scoring.make(match, -1, -3, -2)


def _hip_scoring(affine, match=2):
    return hipkernel.Scoring.make(*((match,) + (AFFINE if affine else LINEAR)[1:]))


def _engine(R, F, band, affine, match=2, alignments=1):
    eng = hipkernel.Engine(R, F, _hip_scoring(affine, match))
    eng.set_band_width(band)
    eng.set_band_alignments(alignments)
    eng.set_band_nw(1)
    return eng


def _shape(R, F, band, affine, match=2):
    eng = _engine(R, F, band, affine, match)
    d = eng.describe(NW, 1)
    eng.close()
    assert d["band_nw"] == 1
    return d["band_block_rows"], d["band_col_align"]


def _check_plugin(reads, refs, band, affine, expect_fill=None, match=2):
    R, F = reads.shape[1], refs.shape[1]
    sc = _scoring(affine, match)
    with _plugin(R, F, band, affine, match) as hip:
        rows, idx = hip.compute_alignments(NW, reads, refs)
        ran = hip.last_ran()
        scores = hip.score_alignments(NW, reads, refs)
        ran_score = hip.last_ran()
    block_rows, col_align = _shape(R, F, band, affine, match)
    exp_scores = bnr.score_banded_nw(reads, refs, band, sc, block_rows, col_align, affine=affine)
    print("band_nw", (R, F, band, affine), "block", (block_rows, col_align), ran["ran_align_fill"], ran_score["ran_score_cells"],
          "score mismatches", int((scores.astype(np.int64) != np.minimum(exp_scores, 32767)).sum()))
    assert np.array_equal(scores.astype(np.int64), np.minimum(exp_scores, 32767)), (block_rows, col_align)
    assert ran_score["ran_score_cells"] == "int32", ran_score
    exp_rows, exp_idx = bnr.align_banded_nw(reads, refs, band, sc, block_rows, col_align, affine=affine)
    bad = [p for p in range(len(reads)) if not (np.array_equal(rows[p], exp_rows[p]) and np.array_equal(idx[p], exp_idx[p]))]
    assert not bad, (block_rows, col_align, bad[:8], idx[bad[0]], exp_idx[bad[0]])
    if expect_fill:
        assert ran["ran_align_fill"] == expect_fill, ran
    return block_rows, col_align


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("R,F,n,band,seed,fill", [(150, 500, 24, 32, 1, "strip_band"), (400, 450, 16, 16, 2, "strip_band"),
                                                  (1000, 1300, 8, 64, 3, "strip_band"), (3000, 2800, 6, 64, 4, "strip_wide_band"),
                                                  (3000, 2800, 6, 512, 5, "strip_wide_band")])
def test_banded_nw_matches_the_restatement(affine, R, F, n, band, seed, fill):
    reads, refs = _pairs(n, R, F, seed)
    _check_plugin(reads, refs, band, affine, expect_fill=fill)


@pytest.mark.parametrize("affine", [False, True])
def test_shifted_insertions(affine):
    reads, refs = shifted_insertion_pairs(n=12)
    _check_plugin(reads, refs, 64, affine, expect_fill="strip_band")


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("R,F,n,band,seed", [(150, 500, 24, 32, 1), (400, 450, 16, 16, 2), (1000, 1300, 8, 64, 3), (3000, 2800, 6, 64, 4),
                                             (3000, 2800, 6, 512, 5), (1200, 1200, 8, 64, 0)])
def test_strip_blocks_under_no_band_chain(affine, R, F, n, band, seed, monkeypatch):
    """The same shapes and bands with the chain switched off: score_long_kernel<..., NWBAND> and the (160, 4) windows."""
    debug_switches(monkeypatch, no_band_chain=1)
    reads, refs = shifted_insertion_pairs(n=n, seed=4) if seed == 0 else _pairs(n, R, F, seed)
    assert _check_plugin(reads, refs, band, affine) == (160, 4)


@pytest.mark.parametrize("affine", [False, True])
def test_wide_band_is_the_unbanded_oracle(affine):
    R, F = 700, 900
    reads, refs = _pairs(16, R, F, 5)
    sc = _scoring(affine)
    with _plugin(R, F, 2 * max(R, F), affine) as hip:
        rows, idx = hip.compute_alignments(NW, reads, refs)
        scores = hip.score_alignments(NW, reads, refs)
    exp_rows, exp_idx = cpu_ref.align(NW, reads, refs, sc, threads=4, affine=affine, wide=True)
    assert np.array_equal(idx, exp_idx) and np.array_equal(rows, exp_rows)
    assert np.array_equal(scores, cpu_ref.score(NW, reads, refs, sc, threads=4, affine=affine, wide=True))


@pytest.mark.parametrize("affine", [False, True])
def test_int32_cells(affine):
    """match 20 on 2,000-base reads: cells leave int16, the banded strips run on int32 cells."""
    reads, refs = synth.make_pairs(4, 2000, 2000, seed=6, sub_rate=0.02, indel_rate=0.002)
    _check_plugin(reads, refs, 128, affine, expect_fill="strip_wide_band", match=20)


@pytest.mark.parametrize("R,F,fill", [(2729, 2729, "strip_band"), (2729, 2730, "strip_wide_band")])
def test_both_sides_of_the_int16_rule(R, F, fill):
    """band_nw_int16_ok (cell_rules.h; tests/band_nw_rules_check.cpp pins the edge): linear 2 / -1 / -3 / -2 keeps the packed int16
    strips up to R + F = 5,458."""
    reads, refs = _pairs(4, R, F, 30)
    _check_plugin(reads, refs, 64, False, expect_fill=fill)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_small_calls_and_device_entry_point(n):
    R, F, band = 150, 500, 16
    reads, refs = _pairs(n, R, F, 20 + n)
    shape = _shape(R, F, band, False)
    exp_rows, exp_idx = bnr.align_banded_nw(reads, refs, band, _scoring(False), *shape)
    exp_scores = bnr.score_banded_nw(reads, refs, band, _scoring(False), *shape)
    with _plugin(R, F, band, False) as hip:
        rows, idx = hip.compute_alignments(NW, reads, refs)
        assert hip.last_ran()["ran_align_fill"] == "strip_band"
    assert np.array_equal(idx, exp_idx) and np.array_equal(rows, exp_rows)
    eng = _engine(R, F, band, False)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    d_rows, d_idx = eng.align_device(NW, d_reads, d_refs)
    d_scores = eng.score_device(NW, d_reads, d_refs)
    torch.cuda.synchronize()
    assert eng.describe(NW, n)["ran_align_fill"] == "strip_band"
    eng.close()
    assert np.array_equal(d_idx.cpu().numpy(), exp_idx) and np.array_equal(d_rows.cpu().numpy(), exp_rows)
    assert np.array_equal(d_scores.cpu().numpy().astype(np.int64), exp_scores)


def test_shards_honour_the_key():
    R, F, band = 1200, 1200, 64
    reads, refs = shifted_insertion_pairs(n=9, seed=7)
    shape = _shape(R, F, band, False)
    exp_rows, exp_idx = bnr.align_banded_nw(reads, refs, band, _scoring(False), *shape)
    exp_scores = bnr.score_banded_nw(reads, refs, band, _scoring(False), *shape)
    with _plugin(R, F, band, False, hip_devices=3) as hip:
        rows, idx = hip.compute_alignments(NW, reads, refs)
        scores = hip.score_alignments(NW, reads, refs)
    assert np.array_equal(idx, exp_idx) and np.array_equal(rows, exp_rows)
    assert np.array_equal(scores.astype(np.int64), exp_scores)


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("ckpt", [0, 1])
def test_cigar_records_behind_the_banded_walk(affine, ckpt):
    """valign_hip_align_cigar_device: records and ops of the restated rows (an empty alignment among them), trace_checkpoints
    on or off."""
    R, F, band = 1000, 1300, 64
    reads, refs = _pairs(8, R, F, 40)
    refs[3, 0] = 0                                   # last_ref = -1 while the end row's window starts beyond column 0: empty
    sc = _scoring(affine)
    shape = _shape(R, F, band, affine)
    rows, idx = bnr.align_banded_nw(reads, refs, band, sc, *shape, affine=affine)
    assert not rows[3].any()
    eng = _engine(R, F, band, affine)
    eng.set_trace_checkpoints(ckpt)
    for extended in (False, True):
        exp = cigar_ref.expected(rows, idx, sc, reads, refs, extended=extended, affine=affine)
        recs, ops = eng.align_cigar_device(NW, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda(), extended=extended, ops_stride=R + F)
        torch.cuda.synchronize()
        recs, ops = recs.cpu().numpy().view(hipkernel.aln_dtype()).reshape(-1), ops.cpu().numpy().view(np.uint32)
        cigar_ref.check(recs, lambda p: ops[p, :recs["n_ops"][p]], exp, reads, refs, ("band_nw", affine, extended))
    assert eng.describe(NW, 8)["ran_align_fill"] == "strip_band"
    eng.close()


def test_refusals():
    R, F = 300, 300
    reads, refs = _pairs(4, R, F, 8)
    eng = hipkernel.Engine(R, F, _hip_scoring(False))
    with pytest.raises(hipkernel.HipKernelError, match="band_nw must be 0 or 1"):
        eng.set_band_nw(2)
    eng.close()
    with pytest.raises(host.PluginError, match="band_nw must be 0 or 1"):
        _plugin(R, F, 32, False, band_nw=2).__enter__()
    # the narrow band: 2 * 1 + 1 = 3 < ceil(500 / 150) = 4
    r2, f2 = _pairs(4, 150, 500, 9)
    with _plugin(150, 500, 2, False) as hip:
        with pytest.raises(host.PluginError, match="do not connect"):
            hip.score_alignments(NW, r2, f2)
        with pytest.raises(host.PluginError, match="do not connect"):
            hip.compute_alignments(NW, r2, f2)
        hip.score_alignments(0, r2, f2)              # Smith-Waterman does not read the key
    with _plugin(R, F, 32, False, traceback_policy=1) as hip:
        with pytest.raises(host.PluginError, match="traceback_policy"):
            hip.compute_alignments(NW, reads, refs)
    # band_nw = 0: the two existing messages, unchanged
    with _plugin(R, F, 32, False, band_nw=0) as hip:
        with pytest.raises(host.PluginError, match="band_width applies to Smith-Waterman scores only"):
            hip.score_alignments(NW, reads, refs)
        with pytest.raises(host.PluginError, match="band_alignments applies to Smith-Waterman alignments only"):
            hip.compute_alignments(NW, reads, refs)


def test_key_without_band_alignments_keeps_unbanded_alignments():
    R, F = 1200, 1200
    reads, refs = shifted_insertion_pairs(n=6, seed=11)
    sc = _scoring(False)
    with _plugin(R, F, 64, False, band_alignments=0) as hip:
        rows, idx = hip.compute_alignments(NW, reads, refs)
    exp_rows, exp_idx = cpu_ref.align(NW, reads, refs, sc, threads=4, wide=True)
    assert np.array_equal(idx, exp_idx) and np.array_equal(rows, exp_rows)


def test_pointer_stream_shrinks_with_the_band():
    """align_ptr_bytes_per_pair of the plan at 10 kbp x 10 kbp, band 512: at most 1/5 of the unbanded plan's (two pairs each)."""
    R = F = 10000
    reads, refs = synth.make_pairs(2, R, F, seed=12, sub_rate=0.05)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    per_pair = {}
    for on in (0, 1):
        eng = _engine(R, F, 512, False, alignments=on)
        eng.align_device(NW, d_reads, d_refs)
        torch.cuda.synchronize()
        d = eng.describe(NW, 2)
        assert d["band_alignments"] == on and d["band_nw"] == 1
        per_pair[on] = d["align_ptr_bytes_per_pair"]
        eng.close()
    print("align_ptr_bytes_per_pair", per_pair)
    assert 0 < per_pair[1] * 5 <= per_pair[0], per_pair
