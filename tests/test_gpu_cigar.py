"""The compact result format on the GPU (valign_hip_align_cigar_device / _host): records and ops encoded on the device behind
every alignment route.  Expected values come from the oracle's rows (cpu_ref.align, band_align_ref) through tests/cigar_ref.py,
never from the library's own row output.

Kinds of pin (cigar_ref.expected / check):
  * ops, their text, n_ops and score: every case, against the oracle's rows;
  * degapped rows == read[read_begin:read_end] / ref[ref_begin:ref_end]: every case;
  * the four coordinates against an INDEPENDENT end cell: Smith-Waterman under the default policy on every route
    (band_align_ref's walk over a band wider than the matrix -- for the banded route, over the engine's own block band); the NW
    variant on the fused route (64 x 128), the register route (150 x 500, the first 40 pairs) and the smallest strip shape
    (2049 x 300, 3 pairs) through ckpt_align_ref._forward;
  * no independent end cell -- the properties above only: traceback_policy = 1 (its end-cell rules differ from the plain-Python
    statements), and the NW variant at 3000 x 3500 / 2000 x 2000 (plain Python would take minutes).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import band_align_ref as bar
import cigar_ref
from conftest import debug_switches
from oracle import cpu_ref
from versalignlib_amd import hipkernel, host, synth

pytestmark = pytest.mark.gpu

AFF = (-5, -1, -4, -2)


def _scorings(affine, match=2, gap_ref=-3):
    if affine:
        return hipkernel.Scoring.make(match, -1, -3, -3, *AFF), cpu_ref.Scoring.make(match, -1, -3, -3, *AFF)
    return hipkernel.Scoring.make(match, -1, -3, gap_ref), cpu_ref.Scoring.make(match, -1, -3, gap_ref)


def _pairs(n, R, F, seed):
    return synth.make_pairs(n, R, F, seed=seed, sub_rate=0.1, indel_rate=0.02, n_run_frac=0.1, short_frac=0.15, lowercase_frac=0.05,
                            junk_frac=0.04)


def _device(eng, opt, reads, refs, extended, stride=None):
    stride = stride or reads.shape[1] + refs.shape[1]
    recs, ops = eng.align_cigar_device(opt, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda(), extended=extended, ops_stride=stride)
    torch.cuda.synchronize()
    return recs.cpu().numpy().view(hipkernel.aln_dtype()).reshape(-1), ops.cpu().numpy().view(np.uint32)


def _check_device(eng, opt, reads, refs, exp_by_ext, what):
    for extended, exp in exp_by_ext.items():
        recs, ops = _device(eng, opt, reads, refs, extended)
        cigar_ref.check(recs, lambda p: ops[p, :recs["n_ops"][p]], exp, reads, refs, (what, "device", extended))


def _check_host(eng, opt, reads, refs, exp_by_ext, what, threads=2):
    for extended, exp in exp_by_ext.items():
        recs, ops, offsets = eng.align_cigar_host(opt, reads, refs, extended=extended, threads=threads)
        assert offsets[0] == 0 and np.array_equal(np.diff(offsets), recs["n_ops"].astype(np.int64)) and len(ops) == offsets[-1]
        cigar_ref.check(recs, lambda p: ops[offsets[p]:offsets[p + 1]], exp, reads, refs, (what, "host", extended))


def _expected(rows, idx, osc, reads, refs, affine=False, ends=None):
    return {ext: cigar_ref.expected(rows, idx, osc, reads, refs, extended=ext, affine=affine, ends=ends) for ext in (False, True)}


def _ends(opt, reads, refs, osc, affine, nw_pairs=None):
    """independent end cells (module docstring); None where plain Python would take too long"""
    if opt == host.SW:
        return cigar_ref.end_cells_sw(reads, refs, osc, affine)
    if nw_pairs is None:
        return None
    return cigar_ref.end_cells_nw(reads[:nw_pairs], refs[:nw_pairs], osc, affine)


@pytest.mark.parametrize("opt", [host.SW, host.NW])
def test_fused_small_call(opt):
    """64 x 128 through the host entry point: one launch fills, walks and hands the end cells out."""
    R, F, n = 64, 128, 300
    reads, refs = _pairs(n, R, F, 3)
    sc, osc = _scorings(False)
    rows, idx = cpu_ref.align(opt, reads, refs, osc, threads=4)
    exp = _expected(rows, idx, osc, reads, refs, ends=_ends(opt, reads, refs, osc, False, nw_pairs=n))
    eng = hipkernel.Engine(R, F, sc)
    _check_host(eng, opt, reads, refs, exp, "fused")
    assert eng.describe(opt, n)["ran_align_fill"] == "fused_tag"
    if opt == host.SW:
        recs, _, _ = eng.align_cigar_host(opt, reads, refs)
        assert np.array_equal(recs["score"], cpu_ref.score(host.SW, reads, refs, osc, threads=4).astype(np.int32))
    eng.close()


@pytest.mark.parametrize("opt", [host.SW, host.NW])
@pytest.mark.parametrize("affine", [False, True])
def test_register_path(opt, affine):
    """150 x 500, linear and affine gaps, device and host entry points."""
    R, F = 150, 500
    n = 203 if opt == host.SW else 40
    reads, refs = _pairs(n, R, F, 5 + opt)
    sc, osc = _scorings(affine)
    rows, idx = cpu_ref.align(opt, reads, refs, osc, threads=4, affine=affine)
    exp = _expected(rows, idx, osc, reads, refs, affine, ends=_ends(opt, reads, refs, osc, affine, nw_pairs=n))
    eng = hipkernel.Engine(R, F, sc)
    _check_device(eng, opt, reads, refs, exp, ("register", affine))
    ran = eng.describe(opt, n)["ran_align_fill"]
    assert ran not in ("none", "fused_tag") and not ran.startswith("strip"), ran
    _check_host(eng, opt, reads, refs, exp, ("register", affine))
    if opt == host.SW:                       # two oracle paths agree through the library: the rescored alignment is the SW score
        recs, _ = _device(eng, opt, reads, refs, False)
        assert np.array_equal(recs["score"], cpu_ref.score(host.SW, reads, refs, osc, threads=4, affine=affine).astype(np.int32))
    eng.close()


@pytest.mark.parametrize("opt", [host.SW, host.NW])
def test_sse_traceback_policy(opt):
    """traceback_policy = 1: ops, n_ops, score and the degapped-rows property against cpu_ref.align(policy="sse"); no
    independent end cell (module docstring)."""
    R, F, n = 150, 500, 120
    reads, refs = _pairs(n, R, F, 9)
    sc, osc = _scorings(False)
    rows, idx = cpu_ref.align(opt, reads, refs, osc, threads=4, policy="sse")
    exp = _expected(rows, idx, osc, reads, refs)
    eng = hipkernel.Engine(R, F, sc)
    eng.set_traceback_policy(1)
    _check_device(eng, opt, reads, refs, exp, "sse")
    assert "sse" in eng.describe(opt, n)["ran_align_fill"]
    eng.close()


@functools.lru_cache(maxsize=None)
def _strip_case(opt):
    R, F, n = 3000, 3500, 5
    reads, refs = _pairs(n, R, F, 11)
    _, osc = _scorings(False)
    rows, idx = cpu_ref.align(opt, reads, refs, osc, threads=8)
    return reads, refs, _expected(rows, idx, osc, reads, refs, ends=_ends(opt, reads, refs, osc, False))


@pytest.mark.parametrize("opt", [host.SW, host.NW])
@pytest.mark.parametrize("ckpt", [0, 1])
def test_row_strips(opt, ckpt):
    """3000 x 3500, an odd pair count: the full-pointer strips and the checkpointed traceback."""
    reads, refs, exp = _strip_case(opt)
    eng = hipkernel.Engine(3000, 3500, _scorings(False)[0])
    eng.set_trace_checkpoints(ckpt)
    _check_device(eng, opt, reads, refs, exp, ("strip", ckpt))
    assert eng.describe(opt, 5)["ran_align_fill"] == ("strip_ckpt" if ckpt else "strip")
    _check_host(eng, opt, reads, refs, {True: exp[True]}, ("strip", ckpt))
    eng.close()


def test_smallest_strip_shape_nw_end_cells():
    """2049 x 300, 3 pairs: the NW variant's coordinates against ckpt_align_ref._forward's end cell on a strip route."""
    R, F, n = 2049, 300, 3
    reads, refs = _pairs(n, R, F, 13)
    reads[1, 1500:] = 0                       # a read that ends early: the end cell sits in an earlier strip
    sc, osc = _scorings(False)
    rows, idx = cpu_ref.align(host.NW, reads, refs, osc, threads=4)
    exp = _expected(rows, idx, osc, reads, refs, ends=_ends(host.NW, reads, refs, osc, False, nw_pairs=n))
    for ckpt in (0, 1):
        eng = hipkernel.Engine(R, F, sc)
        eng.set_trace_checkpoints(ckpt)
        _check_device(eng, host.NW, reads, refs, exp, ("2049x300", ckpt))
        assert eng.describe(host.NW, n)["ran_align_fill"] == ("strip_ckpt" if ckpt else "strip")
        eng.close()


@pytest.mark.parametrize("opt", [host.SW, host.NW])
def test_int32_strips(opt):
    """match = 20 on 2,000-base reads leaves int16: strip_wide."""
    R = F = 2000
    reads, refs = synth.make_pairs(5, R, F, seed=53, sub_rate=0.02, indel_rate=0.002)
    sc, osc = _scorings(False, match=20)
    rows, idx = cpu_ref.align(opt, reads, refs, osc, threads=8, wide=True)
    exp = _expected(rows, idx, osc, reads, refs, ends=_ends(opt, reads, refs, osc, False))
    eng = hipkernel.Engine(R, F, sc)
    _check_device(eng, opt, reads, refs, exp, "strip_wide")
    assert eng.describe(opt, 5)["ran_align_fill"] == "strip_wide"
    eng.close()


@pytest.mark.parametrize("affine", [False, True])
def test_banded_alignments(affine):
    """band_alignments = 1: the oracle is band_align_ref on the engine's block band; its walk gives the end cells."""
    R, F, n, band = 3000, 2800, 6, 64
    reads, refs = synth.make_pairs(n, R, F, seed=2, sub_rate=0.1, indel_rate=0.01, n_run_frac=0.2, short_frac=0.15, lowercase_frac=0.05, junk_frac=0.05)
    sc, osc = _scorings(affine, gap_ref=-2)
    eng = hipkernel.Engine(R, F, sc)
    eng.set_band_width(band)
    eng.set_band_alignments(1)
    d = eng.describe(0, n)
    rows, idx, walked = bar.align_banded_sw(reads, refs, band, osc, d["band_block_rows"], d["band_col_align"], affine=affine, paths=True)
    ends = np.array([w[0] if w else (-1, -1) for w in walked], np.int64).reshape(n, 2)
    exp = _expected(rows, idx, osc, reads, refs, affine, ends=ends)
    _check_device(eng, host.SW, reads, refs, exp, ("band", affine))
    assert eng.describe(0, n)["ran_align_fill"] == "strip_band"
    eng.close()


def _block_expected(opt, reads, refs, osc):
    rows, idx = cpu_ref.align(opt, reads, refs, osc, threads=8)
    ends = _ends(opt, reads, refs, osc, False) if opt == host.SW else None
    return cigar_ref.expected(rows, idx, osc, reads, refs, extended=True, ends=ends)


@pytest.mark.parametrize("opt", [host.SW, host.NW])
def test_parts_and_chunks(monkeypatch, opt):
    """A small pointer scratch cuts the call into parts, a small rows scratch and small host chunks into chunks: the end
    cells of later parts must not leak into earlier pairs.  Twice on the same engine, device and host entry points."""
    debug_switches(monkeypatch, cigar_rows_mb=2, align_chunk_bytes=2 << 20)
    R, F, blk, reps = 150, 500, 1019, 5
    reads, refs = _pairs(blk, R, F, 17)
    sc, osc = _scorings(False)
    exp = _block_expected(opt, reads, refs, osc)
    all_reads, all_refs = np.tile(reads, (reps, 1)), np.tile(refs, (reps, 1))
    eng = hipkernel.Engine(R, F, sc)
    eng.set_pointer_scratch_cap_mb(8)
    for _ in range(2):
        recs, ops = _device(eng, opt, all_reads, all_refs, True, stride=R + F)
        recs_h, ops_h, offsets = eng.align_cigar_host(opt, all_reads, all_refs, extended=True, threads=3)
        for r in range(reps):
            lo = r * blk
            cigar_ref.check(recs[lo:lo + blk], lambda p: ops[lo + p, :recs["n_ops"][lo + p]], exp, reads, refs, ("parts", r))
            cigar_ref.check(recs_h[lo:lo + blk], lambda p: ops_h[offsets[lo + p]:offsets[lo + p + 1]], exp, reads, refs, ("chunks", r))
    eng.close()


def test_batch_beyond_the_overlap_split():
    """142,730 pairs of 150 x 500 (1.07e10 cells): the 7/8 + 1/8 cut with the walk of one part beside the fill of the next;
    the encoder runs behind each part's walk on the helper stream.  Results repeat with the block and equal the oracle's."""
    R, F, blk, reps, stride = 150, 500, 2039, 70, 112
    reads, refs = synth.make_pairs(blk, R, F, seed=77, indel_rate=0.01, junk_frac=0.02)
    sc, osc = _scorings(False)
    eng = hipkernel.Engine(R, F, sc)
    d_reads = torch.from_numpy(reads).cuda().repeat(reps, 1).contiguous()
    d_refs = torch.from_numpy(refs).cuda().repeat(reps, 1).contiguous()
    for opt in (host.SW, host.NW):
        exp = _block_expected(opt, reads, refs, osc)
        assert exp["n_ops"].max() <= stride
        for _ in range(2):
            ops = torch.full((blk * reps, stride), -1, dtype=torch.int32, device="cuda")
            recs = torch.empty((blk * reps, 6), dtype=torch.int32, device="cuda")
            eng.align_cigar_device(opt, d_reads, d_refs, extended=True, ops_stride=stride, out=(recs, ops))
        torch.cuda.synchronize()
        recs, ops = recs.view(reps, blk, 6), ops.view(reps, blk, stride)
        assert bool((recs == recs[0:1]).all()) and bool((ops == ops[0:1]).all())
        r0 = recs[0].cpu().numpy().view(hipkernel.aln_dtype()).reshape(-1)
        o0 = ops[0].cpu().numpy().view(np.uint32)
        cigar_ref.check(r0, lambda p: o0[p, :r0["n_ops"][p]], exp, reads, refs, ("overlap", opt))
    eng.close()


def test_ops_stride_overflow_is_per_pair():
    """ops_stride smaller than some pairs' n_ops: those pairs store their first ops_stride ops, n_ops is the true count and
    nothing is written past a pair's ops (sentinel)."""
    R, F, n, stride = 150, 500, 301, 3
    reads, refs = _pairs(n, R, F, 23)
    sc, osc = _scorings(False)
    rows, idx = cpu_ref.align(host.SW, reads, refs, osc, threads=4)
    exp = cigar_ref.expected(rows, idx, osc, reads, refs, extended=True)
    assert (exp["n_ops"] > stride).any() and (exp["n_ops"] < stride).any()
    eng = hipkernel.Engine(R, F, sc)
    sentinel = 0x7EADBEE5
    ops = torch.full((n, stride), sentinel, dtype=torch.int32, device="cuda")
    recs = torch.empty((n, 6), dtype=torch.int32, device="cuda")
    eng.align_cigar_device(host.SW, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda(), extended=True, ops_stride=stride, out=(recs, ops))
    torch.cuda.synchronize()
    recs = recs.cpu().numpy().view(hipkernel.aln_dtype()).reshape(-1)
    ops = ops.cpu().numpy().view(np.uint32)
    assert np.array_equal(recs["n_ops"].astype(np.int64), exp["n_ops"])
    for p in range(n):
        k = min(stride, len(exp["ops"][p]))
        assert ops[p, :k].tolist() == exp["ops"][p][:k], p
        assert (ops[p, k:] == sentinel).all(), p
    eng.close()


def _raw_host(eng, opt, reads, refs, cap, extended=1, sentinel=None, ops_len=None):
    """ops_len: entries of the ops buffer where that is more than the ops_cap the call is told"""
    n = reads.shape[0]
    rp = (reads.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(reads.shape[1])).astype(np.uint64)
    fp = (refs.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(refs.shape[1])).astype(np.uint64)
    recs = np.zeros(max(n, 1), dtype=hipkernel.aln_dtype())
    ops = np.zeros(max(cap, 1) if ops_len is None else ops_len, np.uint32)
    offsets = np.zeros(n + 1, np.int64)
    if sentinel is not None:
        recs.view(np.int32)[:] = sentinel
        ops.view(np.int32)[:] = sentinel
        offsets[:] = sentinel
    needed = ctypes.c_longlong(-7)
    rc = hipkernel.lib().valign_hip_align_cigar_host(eng._h, opt, n, rp.ctypes.data, fp.ctypes.data, extended, recs.ctypes.data, ops.ctypes.data,
                                                      cap, offsets.ctypes.data, ctypes.byref(needed), 2)
    return rc, recs, ops, offsets, needed.value


def test_host_entry_point_contract():
    """Host results equal the device's; ops_cap one short fails with the exact total and complete recs / offsets, the retry
    succeeds; n = 0; opt = 2 writes nothing; bad arguments are refused with a message."""
    R, F, n = 150, 500, 2500                 # beyond the direct call: the chunk pipeline
    reads, refs = _pairs(n, R, F, 29)
    sc, _ = _scorings(False)
    eng = hipkernel.Engine(R, F, sc)
    for opt in (host.SW, host.NW):
        d_recs, d_ops = _device(eng, opt, reads, refs, True)
        recs, ops, offsets = eng.align_cigar_host(opt, reads, refs, extended=True, threads=4)
        assert np.array_equal(recs, d_recs)
        assert all(np.array_equal(ops[offsets[p]:offsets[p + 1]], d_ops[p, :d_recs["n_ops"][p]]) for p in range(n))
        total = int(offsets[n])
        rc, recs2, _, offsets2, needed = _raw_host(eng, opt, reads, refs, total - 1)
        assert rc != 0 and needed == total and "ops_cap" in hipkernel._err()
        assert np.array_equal(recs2, recs) and np.array_equal(offsets2, offsets)
        rc, recs3, ops3, offsets3, needed = _raw_host(eng, opt, reads, refs, total)
        assert rc == 0 and needed == total and np.array_equal(ops3[:total], ops) and np.array_equal(offsets3, offsets) and np.array_equal(recs3, recs)
    rc, _, _, offsets0, needed = _raw_host(eng, 0, reads[:0], refs[:0], 4, sentinel=-3)
    assert rc == 0 and offsets0[0] == 0 and needed == 0
    rc, recs4, ops4, offsets4, needed = _raw_host(eng, 2, reads[:50], refs[:50], 64, sentinel=-3)
    assert rc == 0 and needed == -7 and (recs4.view(np.int32) == -3).all() and (ops4.view(np.int32) == -3).all() and (offsets4 == -3).all()
    rc, _, _, _, _ = _raw_host(eng, 0, reads[:50], refs[:50], 64, extended=2)
    assert rc != 0 and "extended" in hipkernel._err()
    L = hipkernel.lib()
    one = torch.zeros(8, dtype=torch.int32, device="cuda")
    d_reads, d_refs = torch.from_numpy(reads[:1]).cuda(), torch.from_numpy(refs[:1]).cuda()
    assert L.valign_hip_align_cigar_device(eng._h, 0, 1, d_reads.data_ptr(), d_refs.data_ptr(), 0, one.data_ptr(), one.data_ptr(), 0, None) != 0
    assert "ops_stride" in hipkernel._err()
    assert L.valign_hip_align_cigar_device(eng._h, 0, 1, d_reads.data_ptr(), d_refs.data_ptr(), 0, None, one.data_ptr(), 4, None) != 0
    assert L.valign_hip_align_cigar_device(eng._h, 0, 1, d_reads.data_ptr(), d_refs.data_ptr(), 3, one.data_ptr(), one.data_ptr(), 4, None) != 0
    eng.close()


def test_ops_cap_crossed_between_chunks(monkeypatch):
    """Three chunks of 1 024, 1 024 and 452 pairs on the chunk pipeline, ops_cap passed at a chunk border, one op before it and
    in the last chunk: the return code, the exact need, complete records and offsets, nothing written at or behind ops_cap, only
    the ops of the chunks that still fitted copied back, and the same engine serves the exact retry."""
    debug_switches(monkeypatch, align_chunk_bytes=4096)              # the floor: 1 024 pairs a chunk
    R, F, n, untouched = 150, 500, 2500, -3
    reads, refs = _pairs(n, R, F, 43)
    sc, _ = _scorings(False)
    eng = hipkernel.Engine(R, F, sc)
    recs, ops, offsets = eng.align_cigar_host(host.SW, reads, refs, extended=True, threads=4)
    total, d = int(offsets[n]), eng.describe(0, n)
    # beyond the direct call: the walks ran as kernels of their own, and three op totals crossed
    assert d["ran_align_fill"] not in ("none", "fused_tag") and d["cigar_d2h_bytes"] == 24 * n + 4 * total + 8 * 3, d
    for cap, copied in ((int(offsets[1024]), int(offsets[1024])), (int(offsets[1024]) - 1, 0), (int(offsets[2048]), int(offsets[2048]))):
        assert 0 < cap < total
        rc, recs2, ops2, offsets2, needed = _raw_host(eng, host.SW, reads, refs, cap, sentinel=untouched, ops_len=total)
        assert rc != 0 and needed == total and "ops_cap" in hipkernel._err(), cap
        assert np.array_equal(recs2, recs) and np.array_equal(offsets2, offsets), cap
        assert (ops2.view(np.int32)[cap:] == untouched).all(), cap
        assert eng.describe(0, n)["cigar_d2h_bytes"] == 24 * n + 4 * copied + 8 * 3, cap
        rc, recs3, ops3, offsets3, needed = _raw_host(eng, host.SW, reads, refs, total, sentinel=untouched)
        assert rc == 0 and needed == total and np.array_equal(ops3, ops) and np.array_equal(offsets3, offsets) and np.array_equal(recs3, recs), cap
    eng.close()


def test_describe_reports_the_format_and_what_crossed_pcie():
    """One chunk: records and ops are all there is to send (offsets follow from n_ops on the host), plus the chunk's op total,
    for which 64 bytes are allowed."""
    R, F, n = 150, 500, 3000
    reads, refs = _pairs(n, R, F, 31)
    sc, osc = _scorings(False)
    eng = hipkernel.Engine(R, F, sc)
    recs, ops, offsets = eng.align_cigar_host(host.SW, reads, refs, extended=True, threads=4)
    d = eng.describe(0, n)
    assert d["ran_result_format"] == "cigar"
    assert 24 * n + 4 * int(offsets[n]) <= d["cigar_d2h_bytes"] <= 24 * n + 4 * int(offsets[n]) + 64
    assert 0 < d["cigar_rows_scratch_bytes"] <= 2 * (n * 2 * (R + F) + 64)
    rows, idx = eng.align_host(host.SW, reads, refs, threads=4)
    assert eng.describe(0, n)["ran_result_format"] == "rows"
    _device(eng, host.SW, reads, refs, False)
    assert eng.describe(0, n)["ran_result_format"] == "cigar"
    eng.close()


def test_row_results_before_and_after_are_the_oracles():
    """The new scratch disturbs nothing: compute_alignments-style calls around a cigar call return the oracle's rows."""
    R, F, n = 150, 500, 1500
    reads, refs = _pairs(n, R, F, 37)
    sc, osc = _scorings(False)
    eng = hipkernel.Engine(R, F, sc)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    for opt in (host.SW, host.NW):
        erows, eidx = cpu_ref.align(opt, reads, refs, osc, threads=4)
        for step in range(3):
            rows, idx = eng.align_device(opt, d_reads, d_refs)
            torch.cuda.synchronize()
            assert np.array_equal(idx.cpu().numpy(), eidx) and np.array_equal(rows.cpu().numpy(), erows), (opt, step)
            hrows, hidx = eng.align_host(opt, reads, refs, threads=2)
            assert np.array_equal(hidx, eidx) and np.array_equal(hrows, erows), (opt, step)
            if step == 0:
                _device(eng, opt, reads, refs, True)
            elif step == 1:
                eng.align_cigar_host(opt, reads, refs, extended=True, threads=2)
    eng.close()
