"""Spanned Smith-Waterman scores on the GPU (valign_hip_score_span_device / _host): score, end cell and begin cell of every pair
from two score sweeps, against tests/span_ref.py (numpy, int64 cells, UNCLIPPED reverse sweep, independent of the library).

The route and the bound of the reverse sweep are restated here (`_route`, span_cases.span_ref_length) so that describe()'s
"ran_span" and "span_ref_length" are checked against a prediction, not against themselves."""
import functools

import numpy as np
import pytest
import torch

import placed_ref
import span_cases as sc_
import span_ref
from conftest import debug_switches
from versalignlib_amd import hipkernel

pytestmark = pytest.mark.gpu

FULL = [(8, 8), (16, 10), (32, 10), (64, 8), (64, 16), (64, 32)]


def _route(R, F, match, K, forced):
    if not forced and R > 1024:
        return "strip"
    bits = 2 if K <= 4 else (3 if K <= 8 else 4)
    return "key" if K <= 16 and ((min(R, F) * max(match, 0) + 1) << bits) <= 32000 else "rows"


def _run(eng, reads, refs, opt=0):
    out = eng.score_span_device(opt, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def _host(eng, reads, refs, threads=1):
    got = eng.score_span_host(0, reads, refs, threads=threads)
    assert got.dtype == hipkernel.span_dtype() and got.shape == (len(reads),)
    return np.stack([got[k] for k in hipkernel.span_dtype().names], axis=1).astype(np.int64)


def _check(got, exp, what):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (what, "pairs", bad[:8].tolist(), "got", got[bad[:4]].tolist(), "expected", exp[bad[:4]].tolist())


@functools.lru_cache(maxsize=None)
def _case(R, F, form, seed, n=64):
    reads, refs = sc_.pairs(n, R, F, seed)
    exp = span_ref.spans(reads, refs, sc_.scoring(form), affine=sc_.is_affine(form), chunk=32)
    exp.setflags(write=False)
    return reads, refs, exp


# ---- 1. shapes x gap forms x the default plan and one forced full geometry ----
@pytest.mark.parametrize("R,F", [(12, 20), (33, 70), (40, 9), (64, 128), (150, 500), (20, 120)])
def test_shapes_forms_geometries(R, F):
    forced = next(g for g in FULL if g[0] * g[1] >= R)
    for form in sc_.FORMS:
        reads, refs, exp = _case(R, F, form, 11 * R + F)
        sc = sc_.scoring(form)
        Fr = sc_.span_ref_length(R, F, sc)
        for G, K in ((0, 0), forced):
            eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
            got = _run(eng, reads, refs)
            d = eng.describe(0, 64)
            eng.close()
            _check(got, exp, (R, F, form, G, K))
            assert d["span_ref_length"] == Fr, (R, F, form, d["span_ref_length"], Fr)
            fwd, _, rev = d["ran_span"].partition("/")
            assert d["ran_placed"] == fwd and rev in ("key", "rows"), d["ran_span"]
            if G:               # (forced: both sweeps run on G x K; unforced, each engine picks the geometry of its own shape)
                assert d["ran_span"] == "%s/%s" % (_route(R, F, 2, K, True), _route(R, Fr, 2, K, True)), (R, F, form, d["ran_span"])
                assert d["ran_placed_geometry"] == "%dx%d" % (G, K), (R, F, form, d["ran_placed_geometry"])       # (the forward sweep's; a full geometry carries every form)
    assert sc_.span_ref_length(20, 120, sc_.scoring("sym")) == 33 and sc_.span_ref_length(150, 500, sc_.scoring("sym")) == 249


def test_rows_route_on_64x24():
    R, F = 1000, 200
    for form in ("sym", "aff"):
        reads, refs, exp = _case(R, F, form, 5)
        eng = hipkernel.Engine(R, F, sc_.scoring(form), group_lanes=64, rows_per_lane=24)
        got = _run(eng, reads, refs)
        d = eng.describe(0, 64)
        eng.close()
        _check(got, exp, ("64x24", form))
        assert d["ran_span"] == "rows/rows" and d["span_ref_length"] == 200
        assert d["ran_placed_geometry"] == "64x24", d["ran_placed_geometry"]


@pytest.mark.parametrize("form", ["sym", "aff"])
def test_strip_route(form):
    R, F = 1025, 1300
    reads, refs, exp = _case(R, F, form, R, n=6)
    sc = sc_.scoring(form)
    eng = hipkernel.Engine(R, F, sc)
    got = _run(eng, reads, refs)
    d = eng.describe(0, 6)
    eng.close()
    _check(got, exp, (R, form))
    # prediction: more than 1 024 rows, unforced -> both sweeps on the strips; R + (2 R - 1) // c >= 1300 for c = 3 and c = 2
    c = 2 if form == "aff" else 3
    assert min(F, R + (2 * R - 1) // c) == F
    assert d["ran_span"] == "strip/strip" and d["ran_placed"] == "strip" and d["span_ref_length"] == F


# ---- 2. ties and borders, built by hand ----
@pytest.mark.parametrize("form", ["sym", "aff"])
@pytest.mark.parametrize("R,F,G,K", [(150, 200, 16, 10), (150, 200, 0, 0), (33, 70, 0, 0), (40, 9, 8, 8)])
def test_ties_begin_at_the_later_cell(R, F, G, K, form):
    sc = sc_.tie_scoring(form)
    eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
    for name, (reads, refs, exp) in sc_.tie_batches(R, F).items():
        got = _run(eng, reads, refs)
        _check(got, exp, (name, "by construction"))
        _check(got, span_ref.spans(reads, refs, sc, affine=form == "aff"), (name, "reference"))
    eng.close()


@pytest.mark.parametrize("R,F", [(12, 20), (40, 9), (20, 120), (150, 500)])
def test_borders_and_prefixes_longer_than_the_clip(R, F):
    """end and begin cells in row 0 / column 0 / the last row / the last column; at 20 x 120 and 150 x 500 the end cells in
    the last column have prefixes far longer than span_ref_length (33 / 249 columns)"""
    reads, refs, exp = sc_.border_batch(R, F)
    for form in ("sym", "aff"):
        eng = hipkernel.Engine(R, F, sc_.scoring(form))
        got = _run(eng, reads, refs)
        assert eng.describe(0, 1)["span_ref_length"] == sc_.span_ref_length(R, F, sc_.scoring(form))
        eng.close()
        _check(got, exp, (R, F, form))
    if F >= 120:
        assert (exp[:, 4] > sc_.span_ref_length(R, F, sc_.scoring("sym"))).sum() >= 4


def test_nul_tails_lower_case_and_junk():
    R, F = 150, 500
    rng = np.random.default_rng(9)
    reads, refs = sc_.pairs(64, R, F, 41, lowercase_frac=0.3, junk_frac=0.2)
    reads, refs = reads.copy(), refs.copy()
    for p in range(64):
        tail = int(F * rng.choice([0.0, 0.1, 0.5, 0.9]))
        if tail:
            refs[p, F - tail:] = 0
        cut = int(R * rng.choice([0.0, 0.0, 0.3, 0.8]))
        if cut:
            reads[p, R - cut:] = 0
    refs[8:16, 50:] = 0             # a whole wave whose references are short
    upper = (reads[16:20] >= ord("A")) & (reads[16:20] <= ord("Z"))
    reads[16:20] = np.where(upper, reads[16:20] + 32, reads[16:20])
    refs[20:24, ::7] = ord("#")
    assert (reads == 0).any() and (refs == ord("#")).any() and (reads >= ord("a")).any()
    for form in ("sym", "aff"):
        sc = sc_.scoring(form)
        exp = span_ref.spans(reads, refs, sc, affine=form == "aff", chunk=32)
        eng = hipkernel.Engine(R, F, sc)
        ppw = eng.describe(0, 64)["pairs_per_wave"]
        for n in (64, 1, 7, ppw + 1):
            _check(_run(eng, reads[:n], refs[:n]), exp[:n], (form, n))
        eng.close()
        assert (exp[:, 0] > 0).sum() > 40


# ---- 3. host path, chunks, neighbours ----
@pytest.mark.parametrize("chunks", [False, True])
def test_host_path_equals_device_path(monkeypatch, chunks):
    if chunks:
        debug_switches(monkeypatch, chunk_bytes=200000)               # several chunks, more than the pipeline has slots
    R, F = 64, 128
    reads, refs = sc_.pairs(5000, R, F, 12, indel_rate=0.0)
    for form in ("sym", "aff"):
        eng = hipkernel.Engine(R, F, sc_.scoring(form))
        dev = _run(eng, reads, refs)
        for threads in (1, 4):
            _check(_host(eng, reads, refs, threads), dev, (form, threads, chunks))
        assert eng.describe(0, 5000)["direct_call"] == 0
        eng.set_host_packing(0)
        _check(_host(eng, reads, refs, 2), dev, (form, "raw ASCII", chunks))
        _check(_host(eng, reads[:100], refs[:100], 2), dev[:100], (form, "direct"))        # the direct call
        assert eng.describe(0, 100)["direct_call"] == 1
        eng.close()
    _check(dev[:256], span_ref.spans(reads[:256], refs[:256], sc_.scoring("aff"), affine=True), "device path")


def test_a_call_of_several_internal_chunks_equals_one_chunk(monkeypatch):
    R, F = 150, 500
    reads, refs, exp = _case(R, F, "sym", 11 * R + F)
    sc = sc_.scoring("sym")
    eng = hipkernel.Engine(R, F, sc)
    one = _run(eng, reads, refs)
    whole = eng.describe(0, 64)["span_scratch_bytes"]
    eng.close()
    per_pair = R + sc_.span_ref_length(R, F, sc) + 24
    assert whole >= 64 * per_pair
    debug_switches(monkeypatch, span_scratch_bytes=20 * per_pair)      # 20 pairs a chunk: four chunks, the last one short
    eng = hipkernel.Engine(R, F, sc)
    cut = _run(eng, reads, refs)
    held = eng.describe(0, 64)["span_scratch_bytes"]
    eng.close()
    assert 0 < held <= 20 * per_pair + 64, (held, per_pair)
    _check(cut, one, "chunked against one chunk")
    _check(one, exp, "one chunk")


def test_placed_scores_before_and_after_are_identical_and_streams():
    R, F = 150, 500
    reads, refs, exp = _case(R, F, "affsym", 11 * R + F)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    eng = hipkernel.Engine(R, F, sc_.scoring("affsym"))
    before = eng.score_placed_device(0, d_reads, d_refs).cpu().numpy()
    stream = torch.cuda.Stream()
    out_a = torch.zeros((64, 5), dtype=torch.int32, device="cuda")
    out_b = torch.zeros((64, 5), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.score_span_device(0, d_reads, d_refs, out=out_a, stream=stream)       # two calls back to back on a stream of its own
    eng.score_span_device(0, d_reads, d_refs, out=out_b, stream=stream)
    stream.synchronize()
    after = eng.score_placed_device(0, d_reads, d_refs).cpu().numpy()
    assert eng.describe(0, 64)["ran_placed"] in ("key", "rows")
    eng.close()
    assert np.array_equal(before, after)
    assert np.array_equal(before.astype(np.int64), placed_ref.placed(reads, refs, sc_.scoring("affsym"), affine=True))
    _check(out_a.cpu().numpy().astype(np.int64), exp, "first call")
    _check(out_b.cpu().numpy().astype(np.int64), exp, "second call")


# ---- 4. refusals ----
def test_refusals_and_the_silent_no_op():
    R, F = 64, 128
    reads, refs = sc_.pairs(8, R, F, 1)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()

    def refused(eng, opt, word):
        out = torch.full((8, 5), -7, dtype=torch.int32, device="cuda")
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.score_span_device(opt, d_reads, d_refs, out=out)
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.score_span_host(opt, reads, refs)
        torch.cuda.synchronize()
        d = eng.describe(0, 8)
        assert (out.cpu().numpy() == -7).all() and d["ran_span"] == "none" and d["ran_placed"] == "none"

    sc = sc_.scoring("sym")
    eng = hipkernel.Engine(R, F, sc)
    assert eng.describe(0, 8)["ran_span"] == "none"
    refused(eng, 1, "Smith-Waterman only")
    poisoned = torch.full((8, 5), -7, dtype=torch.int32, device="cuda")
    eng.score_span_device(2, d_reads, d_refs, out=poisoned)             # opt & 0xF > 1 does nothing, as everywhere
    torch.cuda.synchronize()
    assert (poisoned.cpu().numpy() == -7).all()
    assert not eng.score_span_host(2, reads, refs)["score"].any()
    eng.set_traceback_policy(1)
    refused(eng, 0, "traceback_policy")
    eng.set_traceback_policy(0)
    eng.set_score_width(32)
    refused(eng, 0, "score_width")
    eng.set_score_width(0)
    exp = span_ref.spans(reads, refs, sc)
    _check(_run(eng, reads, refs), exp, "after the refusals")
    eng.set_score_width(16)
    _check(_run(eng, reads, refs), exp, "score_width = 16")
    eng.set_score_width(0)
    eng.set_band_width(16)
    refused(eng, 0, "spanned scores are not built for band_width > 0")
    eng.set_band_placed(1)
    refused(eng, 0, "spanned scores are not built for band_width > 0")
    refused(eng, 1, "Smith-Waterman only")                               # an unbanded refusal keeps its own text under a band
    eng.close()
    eng = hipkernel.Engine(R, F, sc_.scoring("sym", match=600))          # 64 x 600 > 32000: the cells can leave int16
    refused(eng, 0, "int16")
    eng.close()
