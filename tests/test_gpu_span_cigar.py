"""Spanned CIGARs on the GPU (valign_hip_align_span_device / _host): the alignment of every pair's span from the span's window,
against tests/span_cigar_ref.py (numpy / plain Python, UNCLIPPED, independent of the library).  Every pair of every case is
compared: the record, n_ops and every op.

What describe()'s "ran_span_cigar" must say is restated here (`_forward`, FILL), so that it is checked against a prediction and
not against itself."""
import ctypes

import numpy as np
import pytest
import torch

import span_cases as sc_
import span_cigar_ref
import span_ref
from conftest import debug_switches
from versalignlib_amd import hipkernel

pytestmark = pytest.mark.gpu

FULL = [(8, 8), (16, 10), (32, 10), (64, 8), (64, 16), (64, 32)]
# the child's fill kernel on a register geometry of at most 16 rows per lane, at these shapes and scores (cell_rules.h fill_choice:
# every range rule holds for min(R, F) x 2 <= 300): the tagged kernels, the lane key in the profile for linear gaps
FILL = {"sym": "tag_prof_key", "lin": "tag_prof_key", "affsym": "affine_tag_sym", "aff": "affine_tag"}
MARKER = -559038737          # 0xDEADBEEF as int32


def _forward(R, F, match, K):
    """the forward sweep's route on a forced geometry of K rows per lane (cell_rules.h placed_choice)"""
    bits = 2 if K <= 4 else (3 if K <= 8 else 4)
    return "key" if K <= 16 and ((min(R, F) * max(match, 0) + 1) << bits) <= 32000 else "rows"


def _device(eng, reads, refs, extended=False, stride=64, opt=0):
    recs, ops = eng.align_span_device(opt, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda(), extended=extended, ops_stride=stride)
    torch.cuda.synchronize()
    return recs.cpu().numpy().astype(np.int64), ops.cpu().numpy().view(np.uint32)


def _check(recs, ops, exp, what):
    """recs int64 [n, 6], ops uint32 [n, stride] of the device entry against span_cigar_ref.expected"""
    bad = np.nonzero((recs != exp["recs"]).any(axis=1))[0]
    assert bad.size == 0, (what, "records of pairs", bad[:8].tolist(), "got", recs[bad[:4]].tolist(), "expected", exp["recs"][bad[:4]].tolist())
    stride = ops.shape[1]
    for p in range(len(recs)):
        want = exp["ops"][p][:stride]
        assert ops[p, :len(want)].tolist() == want, (what, p, "ops", ops[p, :len(want)].tolist(), want)


def _check_packed(recs, ops, offsets, exp, what):
    """the host entry's packed results against span_cigar_ref.expected"""
    got = np.stack([recs[k] for k in hipkernel.aln_dtype().names], axis=1).astype(np.int64)
    bad = np.nonzero((got != exp["recs"]).any(axis=1))[0]
    assert bad.size == 0, (what, "records of pairs", bad[:8].tolist(), got[bad[:4]].tolist(), exp["recs"][bad[:4]].tolist())
    assert offsets[0] == 0 and np.array_equal(np.diff(offsets), exp["recs"][:, 5]), (what, "offsets")
    assert ops.tolist() == [o for pair in exp["ops"] for o in pair], (what, "ops")


# ---- 1. shapes x gap forms x the default plan and one forced full geometry ----
@pytest.mark.parametrize("R,F", [(12, 20), (33, 70), (40, 9), (64, 128), (20, 120), (150, 500)])
def test_shapes_forms_geometries(R, F):
    forced = next(g for g in FULL if g[0] * g[1] >= R)
    for form in sc_.FORMS:
        reads, refs, exp = span_cigar_ref.case(R, F, form)
        sc = sc_.scoring(form)
        d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
        assert exp["recs"][:, 5].max() <= 64
        for G, K in ((0, 0), forced):
            eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
            assert eng.describe(0, 64)["ran_span_cigar"] == "none"
            recs, ops = _device(eng, reads, refs)
            d = eng.describe(0, 64)
            spans = eng.score_span_device(0, d_reads, d_refs).cpu().numpy().astype(np.int64)
            placed = eng.score_placed_device(0, d_reads, d_refs).cpu().numpy().astype(np.int64)
            eng.close()
            _check(recs, ops, exp, (R, F, form, G, K))
            assert np.array_equal(recs[:, :4], spans[:, 1:]), (R, F, form, G, K, "coordinates are score_span_device's")
            assert np.array_equal(recs[:, 4], placed[:, 0]), (R, F, form, G, K, "score is score_placed_device's")
            fwd, _, fill = d["ran_span_cigar"].partition("/")
            assert d["ran_placed"] == fwd and fill == FILL[form], (R, F, form, G, K, d["ran_span_cigar"])
            assert d["ran_result_format"] == "cigar" and d["span_cigar_scratch_bytes"] > 0
            assert fwd == (_forward(R, F, 2, K) if G else fwd) and fwd in ("key", "rows"), (R, F, form, G, K, d["ran_span_cigar"])
    if (R, F) == (20, 120):          # the clip is active: the window is 33 - 59 columns of 120
        assert sorted({sc_.span_ref_length(R, F, sc_.scoring(f)) for f in sc_.FORMS}) == [33, 39, 59]


# ---- 2. ties and borders, built by hand ----
@pytest.mark.parametrize("form", ["sym", "aff"])
@pytest.mark.parametrize("R,F,G,K", [(150, 200, 16, 10), (33, 70, 0, 0), (40, 9, 8, 8)])
def test_ties_that_share_the_end_cell(R, F, G, K, form):
    sc = sc_.tie_scoring(form)
    eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
    for name, (reads, refs, spans) in sc_.tie_batches(R, F).items():
        recs, ops = _device(eng, reads, refs)
        # by construction: the motif alone, m matches, begins at the LATER of the tied begin cells
        assert np.array_equal(recs[:, :4], spans[:, 1:]) and np.array_equal(recs[:, 4], spans[:, 0]), (name, "by construction")
        assert np.array_equal(recs[:, 5], np.ones(len(recs))) and np.array_equal(ops[:, 0], (spans[:, 0] // 2) << 4), (name, "one run of M")
        _check(recs, ops, span_cigar_ref.expected(reads, refs, sc, affine=form == "aff"), (name, "reference"))
    eng.close()


@pytest.mark.parametrize("R,F", [(12, 20), (40, 9), (20, 120), (150, 500)])
def test_borders_and_prefixes_longer_than_the_clip(R, F):
    """alignments at row 0 / column 0 / the last row / the last column; at 20 x 120 and 150 x 500 the end cells in the last
    column have prefixes far longer than the window (33 / 249 columns)"""
    reads, refs, spans = sc_.border_batch(R, F)
    for form in ("sym", "aff"):
        sc = sc_.scoring(form)
        eng = hipkernel.Engine(R, F, sc)
        recs, ops = _device(eng, reads, refs)
        eng.close()
        assert np.array_equal(recs[:, :4], spans[:, 1:]) and np.array_equal(recs[:, 4], spans[:, 0]), (R, F, form, "by construction")
        _check(recs, ops, span_cigar_ref.expected(reads, refs, sc, affine=form == "aff"), (R, F, form))
    if F >= 120:
        assert (spans[:, 4] > sc_.span_ref_length(R, F, sc_.scoring("sym"))).sum() >= 4


# ---- 3. op stores ----
@pytest.mark.parametrize("stride", [1, 3])
def test_ops_stride_stores_the_first_ops_and_nothing_else(stride):
    R, F = 33, 70
    for form in ("lin", "aff"):
        reads, refs, exp = span_cigar_ref.case(R, F, form, extended=True)
        n = len(reads)
        eng = hipkernel.Engine(R, F, sc_.scoring(form))
        recs = torch.full((n, 6), MARKER, dtype=torch.int32, device="cuda")
        ops = torch.full((n, stride), MARKER, dtype=torch.int32, device="cuda")
        eng.align_span_device(0, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda(), extended=True, ops_stride=stride, out=(recs, ops))
        torch.cuda.synchronize()
        eng.close()
        got_recs, got = recs.cpu().numpy().astype(np.int64), ops.cpu().numpy()
        assert np.array_equal(got_recs, exp["recs"]), (form, stride, "records")
        more = 0
        for p in range(n):
            k = min(len(exp["ops"][p]), stride)
            assert got[p, :k].view(np.uint32).tolist() == exp["ops"][p][:k], (form, stride, p, "the first ops in forward order")
            assert (got[p, k:] == MARKER).all(), (form, stride, p, "words past the stored ops")
            more += len(exp["ops"][p]) > stride
        assert more >= 20 and any({7, 8} <= {o & 15 for o in pair} for pair in exp["ops"]), (form, stride, more)


# ---- 4. chunks ----
def test_a_call_of_several_chunks_equals_one_chunk(monkeypatch):
    R, F = 150, 500
    reads, refs, exp = span_cigar_ref.case(R, F, "aff")
    sc = sc_.scoring("aff")
    eng = hipkernel.Engine(R, F, sc)
    one = _device(eng, reads, refs)
    whole = eng.describe(0, 64)["span_cigar_scratch_bytes"]
    eng.close()
    per_pair = 3 * (R + sc_.span_ref_length(R, F, sc)) + 12 + 8
    assert whole >= 64 * per_pair
    debug_switches(monkeypatch, span_cigar_mb=0)           # no room at all: the floor of 16 pairs a chunk, four chunks
    eng = hipkernel.Engine(R, F, sc)
    cut = _device(eng, reads, refs)
    held = eng.describe(0, 64)["span_cigar_scratch_bytes"]
    eng.close()
    assert 0 < held <= 16 * per_pair + 128 and held < whole / 3, (held, whole, per_pair)
    assert np.array_equal(cut[0], one[0]) and one[0][:, 5].max() <= 64
    for p in range(64):
        assert np.array_equal(cut[1][p, :one[0][p, 5]], one[1][p, :one[0][p, 5]]), p
    _check(one[0], one[1], exp, "one chunk")
    _check(cut[0], cut[1], exp, "four chunks")


# ---- 5. row strips, with and without checkpoints ----
@pytest.mark.parametrize("form", ["sym", "aff"])
def test_strips_and_checkpointed_strips(form):
    R, F = 1025, 1300
    reads, refs, exp = span_cigar_ref.case(R, F, form, seed=R, n=6)
    stride = int(exp["recs"][:, 5].max())
    eng = hipkernel.Engine(R, F, sc_.scoring(form))
    plain = _device(eng, reads, refs, stride=stride)
    d = eng.describe(0, 6)
    eng.set_trace_checkpoints(1)
    ckpt = _device(eng, reads, refs, stride=stride)
    d_ckpt = eng.describe(0, 6)
    eng.close()
    # prediction: more than 1 024 rows, unforced -> the forward sweep and the child (1025 x 1300: no clip) on the strips
    assert d["ran_span_cigar"] == "strip/strip" and d_ckpt["ran_span_cigar"] == "strip/strip_ckpt", (d["ran_span_cigar"], d_ckpt["ran_span_cigar"])
    _check(plain[0], plain[1], exp, (form, "strips"))
    _check(ckpt[0], ckpt[1], exp, (form, "checkpointed strips"))
    assert np.array_equal(plain[0], ckpt[0]) and (exp["recs"][:, 5] > 0).all()
    for p in range(6):
        k = int(exp["recs"][p, 5])
        assert np.array_equal(plain[1][p, :k], ckpt[1][p, :k]), (form, p)


# ---- 6. the forward sweep on int32 cells ----
def test_wide_forward_sweep_returns_the_same_records():
    R, F = 33, 70
    for form in ("sym", "aff"):
        reads, refs, exp = span_cigar_ref.case(R, F, form)
        eng = hipkernel.Engine(R, F, sc_.scoring(form))
        eng.set_score_width(32)
        eng.set_placed_wide(1)
        recs, ops = _device(eng, reads, refs)
        d = eng.describe(0, 64)
        eng.close()
        assert d["ran_span_cigar"] == "wide/" + FILL[form], d["ran_span_cigar"]         # the child picks its own cells: int16, tagged
        _check(recs, ops, exp, (form, "placed_wide"))


# ---- 7. host entry ----
def _host_raw(eng, reads, refs, cap, extended=0, threads=2, opt=0, ops_len=None):
    """ops_len: entries of the ops buffer where that is more than the ops_cap the call is told"""
    n = len(reads)
    rp = (reads.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(reads.shape[1] if n else 0)).astype(np.uint64)
    fp = (refs.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(refs.shape[1] if n else 0)).astype(np.uint64)
    recs = np.zeros(n, dtype=hipkernel.aln_dtype())
    ops = np.full(max(cap, 1) if ops_len is None else ops_len, 0xDEADBEEF, np.uint32)
    offsets = np.full(n + 1, -7, np.int64)
    needed = ctypes.c_longlong(-7)
    rc = hipkernel.lib().valign_hip_align_span_host(eng._h, opt, n, rp.ctypes.data, fp.ctypes.data, extended, recs.ctypes.data, ops.ctypes.data,
                                                    cap, offsets.ctypes.data, ctypes.byref(needed), threads)
    return rc, recs, ops, offsets, needed.value


def test_host_entry_equals_device_entry(monkeypatch):
    R, F = 33, 70
    for form in ("lin", "aff"):
        reads, refs, exp = span_cigar_ref.case(R, F, form)
        eng = hipkernel.Engine(R, F, sc_.scoring(form))
        for threads in (1, 4):
            recs, ops, offsets = eng.align_span_host(0, reads, refs, threads=threads)
            _check_packed(recs, ops, offsets, exp, (form, threads))
        d = eng.describe(0, 64)
        total = int(exp["recs"][:, 5].sum())
        assert d["cigar_d2h_bytes"] == 24 * 64 + 4 * total + 8 and d["ran_result_format"] == "cigar", d["cigar_d2h_bytes"]
        assert d["ran_span_cigar"].endswith("/" + FILL[form])
        # n = 0 sets offsets[0] = 0 and nothing else
        rc, _, _, offsets, needed = _host_raw(eng, reads[:0], refs[:0], 0)
        assert rc == 0 and offsets[0] == 0 and needed == 0
        # an ops_cap one below the need: non-zero, the need exact, records and offsets complete
        rc, recs, ops, offsets, needed = _host_raw(eng, reads, refs, total - 1)
        assert rc != 0 and needed == total and "ops_cap" in hipkernel._err()
        got = np.stack([recs[k] for k in hipkernel.aln_dtype().names], axis=1).astype(np.int64)
        assert np.array_equal(got, exp["recs"]) and offsets[0] == 0 and np.array_equal(np.diff(offsets), exp["recs"][:, 5])
        rc, recs, ops, offsets, needed = _host_raw(eng, reads, refs, total)
        assert rc == 0 and needed == total
        _check_packed(recs, ops[:total], offsets, exp, (form, "exact cap"))
        eng.close()


def test_host_pipeline_of_three_chunks(monkeypatch):
    debug_switches(monkeypatch, align_chunk_bytes=4096)              # the floor: 1 024 pairs a chunk
    R, F, n = 33, 70, 2500
    reads, refs = sc_.pairs(n, R, F, 12)
    eng = hipkernel.Engine(R, F, sc_.scoring("affsym"))
    recs, ops = _device(eng, reads, refs)
    h_recs, h_ops, offsets = eng.align_span_host(0, reads, refs, threads=4)
    d = eng.describe(0, n)
    eng.close()
    got = np.stack([h_recs[k] for k in hipkernel.aln_dtype().names], axis=1).astype(np.int64)
    assert np.array_equal(got, recs) and np.array_equal(np.diff(offsets), recs[:, 5]) and recs[:, 5].max() <= 64
    assert h_ops.tolist() == [int(o) for p in range(n) for o in ops[p, :recs[p, 5]]]
    assert d["cigar_d2h_bytes"] == 24 * n + 4 * int(offsets[n]) + 8 * 3, (d["cigar_d2h_bytes"], int(offsets[n]))
    exp = span_cigar_ref.expected(reads[1000:1064], refs[1000:1064], sc_.scoring("affsym"), affine=True)       # (across the first chunk border)
    _check(recs[1000:1064], ops[1000:1064], exp, "pairs 1000 - 1063")


def test_ops_cap_crossed_between_chunks(monkeypatch):
    """The three chunks above with ops_cap passed at a chunk border, one op before it and in the last chunk: the return code, the
    exact need, complete records and offsets, nothing written at or behind ops_cap, only the ops of the chunks that still fitted
    copied back, and the same engine serves the exact retry."""
    debug_switches(monkeypatch, align_chunk_bytes=4096)              # the floor: 1 024 pairs a chunk
    R, F, n = 33, 70, 2500
    reads, refs = sc_.pairs(n, R, F, 13)
    eng = hipkernel.Engine(R, F, sc_.scoring("affsym"))
    recs, ops, offsets = eng.align_span_host(0, reads, refs, threads=4)
    total = int(offsets[n])
    assert eng.describe(0, n)["cigar_d2h_bytes"] == 24 * n + 4 * total + 8 * 3
    for cap, copied in ((int(offsets[1024]), int(offsets[1024])), (int(offsets[1024]) - 1, 0), (int(offsets[2048]), int(offsets[2048]))):
        assert 0 < cap < total
        rc, recs2, ops2, offsets2, needed = _host_raw(eng, reads, refs, cap, ops_len=total)
        assert rc != 0 and needed == total and "ops_cap" in hipkernel._err(), cap
        assert np.array_equal(recs2, recs) and np.array_equal(offsets2, offsets), cap
        assert (ops2[cap:] == 0xDEADBEEF).all(), cap
        assert eng.describe(0, n)["cigar_d2h_bytes"] == 24 * n + 4 * copied + 8 * 3, cap
        rc, recs3, ops3, offsets3, needed = _host_raw(eng, reads, refs, total)
        assert rc == 0 and needed == total and np.array_equal(ops3, ops) and np.array_equal(offsets3, offsets) and np.array_equal(recs3, recs), cap
    eng.close()


# ---- 8. refusals ----
def test_refusals_and_the_silent_no_op():
    R, F = 64, 128
    reads, refs = sc_.pairs(8, R, F, 1)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()

    def refused(eng, opt, word, extended=0, stride=4, host=True):
        recs = torch.full((8, 6), -7, dtype=torch.int32, device="cuda")
        ops = torch.full((8, max(stride, 1)), -7, dtype=torch.int32, device="cuda")
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.align_span_device(opt, d_reads, d_refs, extended=extended, ops_stride=stride, out=(recs, ops))
        torch.cuda.synchronize()
        assert (recs.cpu().numpy() == -7).all() and (ops.cpu().numpy() == -7).all(), word
        assert eng.describe(0, 8)["ran_span_cigar"] == "none", word
        if host:
            rc, h_recs, h_ops, _, _ = _host_raw(eng, reads, refs, 1024, extended=extended, opt=opt)
            assert rc != 0 and word in hipkernel._err() and not h_recs["n_ops"].any() and (h_ops == 0xDEADBEEF).all(), word
            assert eng.describe(0, 8)["ran_span_cigar"] == "none", word

    sc = sc_.scoring("sym")
    eng = hipkernel.Engine(R, F, sc)
    exp = span_cigar_ref.expected(reads, refs, sc)
    refused(eng, 1, "Smith-Waterman only")
    recs = torch.full((8, 6), -7, dtype=torch.int32, device="cuda")
    ops = torch.full((8, 4), -7, dtype=torch.int32, device="cuda")
    eng.align_span_device(2, d_reads, d_refs, out=(recs, ops), ops_stride=4)                 # opt & 0xF > 1 writes nothing and returns 0
    torch.cuda.synchronize()
    assert (recs.cpu().numpy() == -7).all() and (ops.cpu().numpy() == -7).all()
    rc, h_recs, _, offsets, _ = _host_raw(eng, reads, refs, 1024, opt=2)
    assert rc == 0 and not h_recs["n_ops"].any() and (offsets == -7).all()
    _check(*_device(eng, reads, refs), exp, "before the refusals")
    refused(eng, 0, "extended must be 0", extended=2)
    _check(*_device(eng, reads, refs), exp, "a refused call leaves the engine usable")
    refused(eng, 0, "ops_stride must be >= 1", stride=0, host=False)
    eng.set_traceback_policy(1)
    refused(eng, 0, "traceback_policy = 1")
    eng.set_traceback_policy(0)
    eng.set_score_width(32)
    refused(eng, 0, "score_width = 32")
    eng.set_score_width(0)
    eng.set_band_width(16)
    refused(eng, 0, "spanned scores are not built for band_width > 0")
    eng.set_band_placed(1)
    refused(eng, 0, "spanned scores are not built for band_width > 0")
    eng.set_band_width(0)
    _check(*_device(eng, reads, refs), exp, "after the refusals")
    eng.close()


# ---- 9. one engine, interleaved calls, against fresh engines ----
def test_interleaved_calls_equal_fresh_engines():
    R, F = 1025, 1300
    reads, refs, _ = span_cigar_ref.case(R, F, "aff", seed=R, n=6)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    sc = sc_.scoring("aff")

    def span(e):
        return [e.score_span_device(0, d_reads, d_refs).cpu().numpy()]

    def aln_span(e):
        recs, ops = e.align_span_device(0, d_reads, d_refs, ops_stride=128, out=(torch.zeros((6, 6), dtype=torch.int32, device="cuda"),
                                                                                 torch.zeros((6, 128), dtype=torch.int32, device="cuda")))
        return [recs.cpu().numpy(), ops.cpu().numpy(), e.describe(0, 6)["ran_span_cigar"]]

    def aln_cigar(e):
        recs, ops = e.align_cigar_device(0, d_reads, d_refs, ops_stride=128, out=(torch.zeros((6, 6), dtype=torch.int32, device="cuda"),
                                                                                  torch.zeros((6, 128), dtype=torch.int32, device="cuda")))
        return [recs.cpu().numpy(), ops.cpu().numpy(), e.describe(0, 6)["ran_align_fill"]]

    def fresh(call, checkpoints):
        e = hipkernel.Engine(R, F, sc)
        e.set_trace_checkpoints(checkpoints)
        out = call(e)
        e.close()
        return out

    def same(a, b, what):
        assert len(a) == len(b), what
        for x, y in zip(a, b):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (what, x, y)

    eng = hipkernel.Engine(R, F, sc)
    same(span(eng), fresh(span, 0), "score_span first")
    same(aln_span(eng), fresh(aln_span, 0), "align_span after score_span")
    same(aln_cigar(eng), fresh(aln_cigar, 0), "align_cigar after align_span")
    same(span(eng), fresh(span, 0), "score_span after the alignments")
    eng.set_trace_checkpoints(1)
    got = aln_span(eng)
    same(got, fresh(aln_span, 1), "align_span after the key change")
    assert got[2] == "strip/strip_ckpt"
    same(aln_cigar(eng), fresh(aln_cigar, 1), "align_cigar after the key change")
    eng.set_trace_checkpoints(0)
    got = aln_span(eng)
    same(got, fresh(aln_span, 0), "align_span after the key is taken back")
    assert got[2] == "strip/strip"
    eng.close()
