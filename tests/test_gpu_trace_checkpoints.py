"""Checkpointed traceback of long-read alignments (trace_checkpoints = 1, AlignRoute::StripCkpt): a forward pass that keeps
every strip's bottom row and no pointers, then per strip, last to first, a re-fill into one pointer region and a resumable walk.
Results are bit-identical to the full-pointer strips by design; every expected value here comes from the oracle
(cpu_ref.align), never from the library's own key-off path."""
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from versalignlib_amd import build, hipkernel, host, synth
from conftest import debug_switches

pytestmark = pytest.mark.gpu

AFFINE_KEYS = ("score_gap_open_read", "score_gap_extend_read", "score_gap_open_ref", "score_gap_extend_ref")
DEFAULT_AFFINE = (-5, -1, -5, -1)


def _same(got, exp, what):
    rows, idx = got
    erows, eidx = exp
    bad = np.nonzero((np.asarray(idx) != eidx).any(axis=1))[0]
    assert bad.size == 0, (what, "idx", bad[:5], np.asarray(idx)[bad[:3]], eidx[bad[:3]])
    bad = np.nonzero((np.asarray(rows) != erows).any(axis=(1, 2)))[0]
    assert bad.size == 0, (what, "rows", bad[:5])


@functools.lru_cache(maxsize=None)
def _linear_case(R, F, n, seed, gaps):
    reads, refs = synth.make_pairs(n, R, F, seed=seed, indel_rate=0.02, n_run_frac=0.15, short_frac=0.25,
                                   lowercase_frac=0.05, junk_frac=0.03)
    sc = cpu_ref.Scoring.make(2, -1, gaps[0], gaps[1])
    return reads, refs, {opt: cpu_ref.align(opt, reads, refs, sc, threads=8) for opt in (host.SW, host.NW)}


@functools.lru_cache(maxsize=None)
def _affine_case(R, F, n, seed, aff):
    reads, refs = synth.make_pairs(n, R, F, seed=seed, indel_rate=0.03, n_run_frac=0.15, short_frac=0.25,
                                   lowercase_frac=0.05, junk_frac=0.03)
    sc = cpu_ref.Scoring.make(2, -1, -3, -3, *aff)
    exp = {}
    for opt in (host.SW, host.NW):
        wide = opt == host.NW and (min(R, F) + 2) * min(aff) < -15000         # (the oracle's cell width, as test_gpu_long.py)
        exp[opt] = cpu_ref.align(opt, reads, refs, sc, threads=8, affine=True, wide=wide)
    return reads, refs, exp


# strip_k: rows per lane forced through VALIGN_HIP_DEBUG (0: the engine's choice) -- 8 makes many short strips
@pytest.mark.parametrize("strip_k", [0, 8, 12])
@pytest.mark.parametrize("R,F,n,seed", [(3000, 3500, 9, 1), (2500, 700, 11, 2), (2049, 300, 7, 3), (5000, 4000, 4, 4), (4100, 9000, 3, 5)])
@pytest.mark.parametrize("gaps", [(-3, -3), (-2, -4)])
def test_alignments_of_long_reads(monkeypatch, R, F, n, seed, gaps, strip_k):
    """The shapes and scorings of test_gpu_long.py::test_alignments_of_long_reads under the key.  Odd pair counts leave a
    wave half empty."""
    if strip_k:
        debug_switches(monkeypatch, strip_k=strip_k)
    reads, refs, exp = _linear_case(R, F, n, seed, gaps)
    with host.Plugin(build.HIP_PLUGIN, R, F, score_gap_read=gaps[0], score_gap_ref=gaps[1], num_threads=4, trace_checkpoints=1) as hip:
        for opt in (host.SW, host.NW):
            if opt == host.NW and (R + 1) * min(gaps) < -32000:
                continue
            got = hip.compute_alignments(opt, reads, refs, normalise=False)
            assert hip.last_ran()["ran_align_fill"] == "strip_ckpt"
            _same(got, exp[opt], (R, F, opt, gaps, strip_k))


@pytest.mark.parametrize("strip_k", [0, 8, 12])
@pytest.mark.parametrize("R,F,n,seed", [(3000, 3500, 7, 11), (2500, 700, 9, 12), (2049, 300, 5, 13), (4100, 6000, 3, 14)])
@pytest.mark.parametrize("aff", [(-5, -1, -5, -1), (-6, -2, -4, -1), (-3, -3, -3, -3)])
def test_affine_alignments_of_long_reads(monkeypatch, R, F, n, seed, aff, strip_k):
    """... and of test_affine_alignments_of_long_reads: the affine state is carried from round to round."""
    if strip_k:
        debug_switches(monkeypatch, strip_k=strip_k)
    reads, refs, exp = _affine_case(R, F, n, seed, aff)
    with host.Plugin(build.HIP_PLUGIN, R, F, num_threads=4, trace_checkpoints=1, **dict(zip(AFFINE_KEYS, aff))) as hip:
        for opt in (host.SW, host.NW):
            got = hip.compute_alignments(opt, reads, refs, normalise=False)
            assert hip.last_ran()["ran_align_fill"] == "strip_ckpt"
            _same(got, exp[opt], (R, F, opt, aff, strip_k))


@pytest.mark.parametrize("affine", [False, True])
def test_config5_shape(affine):
    """10 kbp x 10 kbp, 3 pairs, default scoring, both algorithms."""
    R = F = 10000
    reads, refs = synth.make_pairs(3, R, F, seed=61, sub_rate=0.1, indel_rate=0.01, n_run_frac=0.3, short_frac=0.34)
    sc = cpu_ref.Scoring.make(2, -1, -3, -3, *DEFAULT_AFFINE) if affine else cpu_ref.Scoring.make()
    keys = dict(zip(AFFINE_KEYS, DEFAULT_AFFINE)) if affine else {}
    with host.Plugin(build.HIP_PLUGIN, R, F, num_threads=4, trace_checkpoints=1, **keys) as hip:
        for opt in (host.SW, host.NW):
            got = hip.compute_alignments(opt, reads, refs, normalise=False)
            assert hip.last_ran()["ran_align_fill"] == "strip_ckpt"
            _same(got, cpu_ref.align(opt, reads, refs, sc, threads=8, affine=affine), ("10k", opt, affine))


def _prefix_reads(n, R, F, seed):
    """Reads that are short prefixes (NUL behind them): Smith-Waterman end cells and the NW variant's last valid row fall in
    early strips, pairs start in different rounds and are idle in the others."""
    reads, refs = synth.make_pairs(n, R, F, seed=seed, sub_rate=0.05, indel_rate=0.01)
    lengths = [0, 1, 40, 700, 1023, 1024, 1025, 1900, 2048, 2500, R - 1, R]
    for p in range(n):
        reads[p, lengths[p % len(lengths)]:] = 0
    return reads, refs


@pytest.mark.parametrize("strip_k", [0, 8])
@pytest.mark.parametrize("affine", [False, True])
def test_ragged_batch(monkeypatch, affine, strip_k):
    if strip_k:
        debug_switches(monkeypatch, strip_k=strip_k)
    R, F, n = 3100, 2900, 25
    reads, refs = _prefix_reads(n, R, F, 31)
    sc = cpu_ref.Scoring.make(2, -1, -3, -3, *DEFAULT_AFFINE) if affine else cpu_ref.Scoring.make()
    keys = dict(zip(AFFINE_KEYS, DEFAULT_AFFINE)) if affine else {}
    with host.Plugin(build.HIP_PLUGIN, R, F, num_threads=4, trace_checkpoints=1, **keys) as hip:
        for opt in (host.SW, host.NW):
            got = hip.compute_alignments(opt, reads, refs, normalise=False)
            assert hip.last_ran()["ran_align_fill"] == "strip_ckpt"
            _same(got, cpu_ref.align(opt, reads, refs, sc, threads=8, affine=affine), ("ragged", opt, affine, strip_k))


@pytest.mark.parametrize("affine", [False, True])
def test_call_of_several_chunks_twice(affine):
    """pointer_scratch_cap_mb so small that the checkpointed plan itself is cut into chunks; two calls on one engine."""
    R, F, n, cap_mb = 3000, 3500, 9, 4
    reads, refs, exp = _affine_case(R, F, 9, 41, DEFAULT_AFFINE) if affine else _linear_case(R, F, 9, 41, (-3, -3))
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(2, -1, -3, -3, *(DEFAULT_AFFINE if affine else ())))
    eng.set_trace_checkpoints(1)
    eng.set_pointer_scratch_cap_mb(cap_mb)
    for _ in range(2):
        for opt in (host.SW, host.NW):
            got = eng.align_host(opt, reads, refs, threads=4)
            d = eng.describe(opt, n)
            assert d["ran_align_fill"] == "strip_ckpt" and d["trace_checkpoints"] == 1
            per_pair = d["align_ptr_bytes_per_pair"] + d["align_ckpt_bytes_per_pair"]
            assert d["align_scratch_bytes"] <= cap_mb << 20 and per_pair * n > 2 * d["align_scratch_bytes"], d     # three chunks or more
            _same(got, exp[opt], ("chunks", opt, affine))
    eng.close()


def test_device_entry_point_plugin_and_shards_agree():
    R, F, n = 2500, 700, 11
    reads, refs, exp = _linear_case(R, F, n, 2, (-3, -3))
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(2, -1, -3, -3))
    eng.set_trace_checkpoints(1)
    for opt in (host.SW, host.NW):
        d_rows, d_idx = eng.align_device(opt, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda())
        torch.cuda.synchronize()
        assert eng.describe(opt, n)["ran_align_fill"] == "strip_ckpt"
        _same((d_rows.cpu().numpy(), d_idx.cpu().numpy()), exp[opt], ("align_device", opt))
    eng.close()
    for shards in (1, 3):
        with host.Plugin(build.HIP_PLUGIN, R, F, num_threads=4, trace_checkpoints=1, hip_devices=shards) as hip:
            for opt in (host.SW, host.NW):
                got = hip.compute_alignments(opt, reads, refs, normalise=False)
                assert hip.last_ran()["ran_align_fill"] == "strip_ckpt"
                _same(got, exp[opt], ("plugin", shards, opt))


def _ran_and_rows(R, F, reads, refs, opt, **keys):
    with host.Plugin(build.HIP_PLUGIN, R, F, num_threads=4, **keys) as hip:
        got = hip.compute_alignments(opt, reads, refs, normalise=False)
        return hip.last_ran()["ran_align_fill"], got


def test_paths_the_key_does_not_cover_run_as_ever():
    """Short reads, a band, int32 cells and traceback_policy = 1 under the key: today's path names, the oracle's results."""
    # 150 x 500: the register path (whatever fill kernel the key-off call names)
    reads, refs = synth.make_pairs(203, 150, 500, seed=51, indel_rate=0.02, n_run_frac=0.05, short_frac=0.08)
    for opt in (host.SW, host.NW):
        ran_off, _ = _ran_and_rows(150, 500, reads, refs, opt)
        ran_on, got = _ran_and_rows(150, 500, reads, refs, opt, trace_checkpoints=1)
        assert ran_on == ran_off and not ran_on.startswith("strip"), (ran_on, ran_off)
        _same(got, cpu_ref.align(opt, reads, refs, threads=8), ("150x500", opt))
    # a band wider than the matrix: the banded strips, the unbanded oracle
    R, F = 700, 900
    reads, refs = synth.make_pairs(16, R, F, seed=52, sub_rate=0.1, indel_rate=0.01)
    ran, got = _ran_and_rows(R, F, reads, refs, host.SW, trace_checkpoints=1, band_width=2 * max(R, F), band_alignments=1)
    assert ran == "strip_band"
    _same(got, cpu_ref.align(host.SW, reads, refs, threads=8, wide=True), "band")
    # match = 20 on 2 000-base reads: int32 cells
    R = F = 2000
    reads, refs = synth.make_pairs(5, R, F, seed=53, sub_rate=0.02, indel_rate=0.002)
    for opt in (host.SW, host.NW):
        ran, got = _ran_and_rows(R, F, reads, refs, opt, trace_checkpoints=1, score_match=20)
        assert ran == "strip_wide"
        _same(got, cpu_ref.align(opt, reads, refs, cpu_ref.Scoring.make(20, -1, -3, -3), threads=8, wide=True), ("int32", opt))
    # traceback_policy = 1 on long reads: the full-pointer strips
    R, F = 3000, 3500
    reads, refs = synth.make_pairs(5, R, F, seed=54, sub_rate=0.12, indel_rate=0.01, n_run_frac=0.3, short_frac=0.2)
    for opt in (host.SW, host.NW):
        ran, got = _ran_and_rows(R, F, reads, refs, opt, trace_checkpoints=1, traceback_policy=1)
        assert ran == "strip"
        _same(got, cpu_ref.align(opt, reads, refs, threads=8, policy="sse"), ("sse", opt))


def test_other_values_are_refused():
    eng = hipkernel.Engine(3000, 500, hipkernel.Scoring.make())
    with pytest.raises(hipkernel.HipKernelError, match="trace_checkpoints must be 0 or 1"):
        eng.set_trace_checkpoints(2)
    eng.close()
    with pytest.raises(host.PluginError, match="trace_checkpoints must be 0 or 1"):
        host.Plugin(build.HIP_PLUGIN, 3000, 500, trace_checkpoints=2)


def test_scratch_shrinks_by_the_derived_factor():
    """10 kbp x 10 kbp, 64 pairs, linear gaps, key off against key on, from describe after the call.  Per pair of pairs the
    off-plan holds S * P bytes of pointers and the on-plan P + (S - 1) * row_dwords * 4, with P = floor((F + 70) / 8) * 64 * K * 4
    and row_dwords = ((F + 71) / 64 + 2) * 64: 51.5 MB against 5.5 MB at K = 16, S = 10 -- a ratio of 9.3 (K = 12: about 12,
    K = 8: about 15).  The factor asked for here, 5, is well inside every plan."""
    R = F = 10000
    n = 64
    reads, refs = synth.make_pairs(n, R, F, seed=71, sub_rate=0.08, indel_rate=0.005)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    seen = {}
    for on in (0, 1):
        eng = hipkernel.Engine(R, F, hipkernel.Scoring.make())
        eng.set_trace_checkpoints(on)
        rows, idx = eng.align_device(host.SW, d_reads, d_refs)
        torch.cuda.synchronize()
        seen[on] = eng.describe(host.SW, n)
        eng.close()
        assert seen[on]["trace_checkpoints"] == on and seen[on]["ran_align_fill"] == ("strip_ckpt" if on else "strip")
        if on:      # (and the alignments are right: the first pairs against the oracle)
            exp = cpu_ref.align(host.SW, reads[:4], refs[:4], threads=8)
            _same((rows[:4].cpu().numpy(), idx[:4].cpu().numpy()), exp, "10k x 64")
    off, on = seen[0], seen[1]
    print("off", off["align_ptr_bytes_per_pair"], off["align_ckpt_bytes_per_pair"], off["align_scratch_bytes"],
          "on", on["align_ptr_bytes_per_pair"], on["align_ckpt_bytes_per_pair"], on["align_scratch_bytes"])
    assert off["align_ckpt_bytes_per_pair"] == 0 and on["align_ckpt_bytes_per_pair"] > 0
    assert 5 * (on["align_ptr_bytes_per_pair"] + on["align_ckpt_bytes_per_pair"]) <= off["align_ptr_bytes_per_pair"], (on, off)
    assert 0 < 5 * on["align_scratch_bytes"] <= off["align_scratch_bytes"], (on, off)
