"""The lane-group CIGAR encoders (cigar_encode_kernel / span_cigar_encode_kernel<16 | 64>, cigar_scan_kernel) on alignments whose
every run boundary is known: the plans of tests/cigar_plans.py, each there for one statement of the encoder.

Expected values come twice, and both must hold: from the plan itself (ops, coordinates, score and op count by construction) and
from the oracle's rows through tests/cigar_ref.py (or the plain-Python reference of the entry point: span_cigar_ref,
extend_align_ref, extend_band_align_ref).  The library's own rows are never the expectation.  tests/test_cigar_plans.py holds
the plans to the oracle without a GPU.

The lane width is the engine's (16 where min(R, F) <= 256, 64 beyond) or forced by the debug switch cigar_lanes; describe()'s
"ran_cigar_lanes" must say which one ran, so a test that forces a width proves that the force took."""
import functools

import numpy as np
import pytest
import torch

import cigar_plans as cp
import cigar_ref
import extend_align_ref as ear
import extend_band_align_ref as ebar
import span_cases
import span_cigar_ref
from conftest import debug_switches
from oracle import cpu_ref
from versalignlib_amd import hipkernel, host

pytestmark = pytest.mark.gpu

WIDTHS = (16, 64)
FORMS = ("lin", "aff")
SHAPES = ((256, 400), (257, 400))         # the last shape of 16 lanes, the first of 64
SENTINEL = 0x7EADBEE5
ALWAYS = ear.INT32_MAX
BONUSES = (-1, ALWAYS)
FIELDS = hipkernel.aln_dtype().names


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _expect(cases, R, F, form):
    """-> reads, refs and, per `extended`, the oracle's expectation (cigar_ref.expected) and the plans' own (ops, recs)"""
    reads, refs = cp.batch(cases, R, F)
    osc = cp.scoring(form, cpu_ref.Scoring.make)
    affine = cp.is_affine(form)
    rows, idx = cpu_ref.align(host.SW, reads, refs, osc, threads=4, affine=affine)
    exp, plan = {}, {}
    for ext in (False, True):
        exp[ext] = cigar_ref.expected(rows, idx, osc, reads, refs, extended=ext, affine=affine)
        plan[ext] = ([cp.ops(c.runs, ext) for c in cases], np.array([cp.record(c, form, ext) for c in cases], np.int64).reshape(len(cases), 6))
        assert exp[ext]["ops"] == plan[ext][0]                  # (tests/test_cigar_plans.py says which plan, where this fails)
    _frozen(reads, refs)
    return reads, refs, exp, plan


@functools.lru_cache(maxsize=None)
def _both_lists(R, F, form):
    """the plans of both widths made for `form`, at one shape: every plan of 64 fits 256 x 400 too"""
    cases = [c for W in WIDTHS for c in cp.for_form(cp.plans(W), form)]
    return (cases,) + _expect(cases, R, F, form)


@functools.lru_cache(maxsize=None)
def _own_list(W, form):
    """the plans of W at the shape where the engine picks W itself"""
    cases = cp.for_form(cp.plans(W), form)
    return (cases,) + _expect(cases, *cp.shape(W), form)


def _engine(monkeypatch, R, F, form, forced=None):
    debug_switches(monkeypatch, cigar_lanes=forced)
    eng = hipkernel.Engine(R, F, cp.scoring(form, hipkernel.Scoring.make))
    assert eng.describe(0, 1)["ran_cigar_lanes"] == 0           # before any CIGAR call
    return eng


def _lanes(R, F, forced):
    return forced or (16 if min(R, F) <= 256 else 64)


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def _outputs(n, stride, extend=False):
    """Result buffers filled with the sentinel: a store the encoder leaves out must not find the right word already there (the
    allocator hands a freed block of an earlier call back)."""
    out = (torch.full((n, 6), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((n, stride), SENTINEL, dtype=torch.int32, device="cuda"))
    return out + (torch.full((n, 5), SENTINEL, dtype=torch.int32, device="cuda"),) if extend else out


def _device(eng, reads, refs, extended, stride):
    recs, ops = eng.align_cigar_device(host.SW, _cuda(reads), _cuda(refs), extended=extended, ops_stride=stride, out=_outputs(len(reads), stride))
    torch.cuda.synchronize()
    return recs.cpu().numpy().view(hipkernel.aln_dtype()).reshape(-1), ops.cpu().numpy().view(np.uint32)


def _as_rows(recs):
    return np.stack([recs[k] for k in FIELDS], axis=1).astype(np.int64)


def _check(recs, ops_of_pair, reads, refs, exp, plan, what):
    """structured recs [n] and the stored ops of each pair against the oracle (cigar_ref.check) and against the plans"""
    cigar_ref.check(recs, ops_of_pair, exp, reads, refs, what)
    got = _as_rows(recs)
    bad = np.nonzero((got != plan[1]).any(axis=1))[0]
    assert bad.size == 0, (what, "records by construction, pairs", bad[:8].tolist(), got[bad[:4]].tolist(), plan[1][bad[:4]].tolist())
    for p, want in enumerate(plan[0]):
        assert [int(x) for x in ops_of_pair(p)] == want, (what, p, "ops by construction")


def _check_host(out, reads, refs, exp, plan, what):
    recs, ops, offsets = out[:3]
    counts = np.array([len(o) for o in plan[0]], np.int64)
    assert offsets[0] == 0 and np.array_equal(np.diff(offsets), counts) and len(ops) == counts.sum(), (what, "offsets against the plans' op counts")
    _check(recs, lambda p: ops[offsets[p]:offsets[p + 1]], reads, refs, exp, plan, what)


def _stride(plan):
    return max(len(o) for o in plan[True][0]) + 1


# ---- 1. both widths on both sides of the rule ----
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("forced", [None, 16, 64])
@pytest.mark.parametrize("R,F", SHAPES)
def test_both_widths_on_both_sides_of_the_rule(monkeypatch, R, F, forced, form):
    """Every plan of both lists through cigar_encode_kernel<the width that is asked for>: the device entry (records + strided
    ops) and the host entry (count pass, scan, emit pass at the scanned offsets), extended and not."""
    cases, reads, refs, exp, plan = _both_lists(R, F, form)
    eng = _engine(monkeypatch, R, F, form, forced)
    for ext in (False, True):
        recs, ops = _device(eng, reads, refs, ext, _stride(plan))
        assert eng.describe(0, len(cases))["ran_cigar_lanes"] == _lanes(R, F, forced), (R, F, forced)
        _check(recs, lambda p: ops[p, :recs["n_ops"][p]], reads, refs, exp[ext], plan[ext], (R, F, forced, form, "device", ext))
        out = eng.align_cigar_host(host.SW, np.array(reads), np.array(refs), extended=ext, threads=2)
        d = eng.describe(0, len(cases))
        assert d["ran_cigar_lanes"] == _lanes(R, F, forced) and d["ran_result_format"] == "cigar", d
        _check_host(out, reads, refs, exp[ext], plan[ext], (R, F, forced, form, "host", ext))
    eng.close()


def test_a_refused_call_reports_no_width(monkeypatch):
    R, F = SHAPES[0]
    cases, reads, refs, exp, plan = _both_lists(R, F, "lin")
    eng = _engine(monkeypatch, R, F, "lin")
    _device(eng, reads[:4], refs[:4], True, 8)
    assert eng.describe(0, 4)["ran_cigar_lanes"] == 16
    eng.set_band_width(64)                  # banded alignments without band_nw: the NW variant is refused
    eng.set_band_alignments(1)
    with pytest.raises(hipkernel.HipKernelError):
        eng.align_cigar_device(host.NW, _cuda(reads[:4]), _cuda(refs[:4]), extended=True, ops_stride=8)
    assert eng.describe(0, 4)["ran_cigar_lanes"] == 0
    eng.set_band_alignments(0)
    eng.set_band_width(0)
    eng.align_span_device(host.SW, _cuda(reads[:4]), _cuda(refs[:4]), extended=True, ops_stride=8)
    torch.cuda.synchronize()
    assert eng.describe(0, 4)["ran_cigar_lanes"] == 16
    eng.set_band_width(64)                  # spanned CIGARs are refused under any band
    with pytest.raises(hipkernel.HipKernelError):
        eng.align_span_device(host.SW, _cuda(reads[:4]), _cuda(refs[:4]), extended=True, ops_stride=8)
    assert eng.describe(0, 4)["ran_cigar_lanes"] == 0
    eng.close()


# ---- 2. four pairs of one wave at 16 lanes ----
def _quads():
    """Groups of four whose column counts are (0, 1, 16, 47) and (0, 28, 35, 61), each in its four rotations: every lane group
    of a wave (gbase 0, 16, 32, 48) holds the longest pair once, its neighbours done steps earlier.  70 pairs: not a multiple
    of 4 (the last wave holds two pairs) nor of 16 (the last block is partial)."""
    W = 16
    by_name = {c.name: c for c in cp.plans(W)}
    quads = [[by_name[k] for k in names] for names in (("nul", "eq1", "eq16", "eq47"), ("nul", "x@15", "alternate", "span2steps"))]
    assert [[cp.columns(c.runs) for c in q] for q in quads] == [[0, 1, W, 3 * W - 1], [0, 28, 2 * W + 3, 61]]
    block = [q[(k + r) % 4] for q in quads for r in range(4) for k in range(4)]
    cases = block + block + block[:6]
    assert len(cases) % 4 and len(cases) % 16 and len(cases) > 16
    for g in range(4):                      # each lane group holds each quad's longest pair
        assert {c.name for c in cases[g::4]} >= {"eq47", "span2steps"}
    return cases


@pytest.mark.parametrize("form", FORMS)
def test_four_pairs_of_one_wave(monkeypatch, form):
    R, F = SHAPES[0]
    cases = _quads()
    reads, refs, exp, plan = _expect(cases, R, F, form)
    eng = _engine(monkeypatch, R, F, form)
    recs, ops = _device(eng, reads, refs, True, _stride(plan))
    assert eng.describe(0, len(cases))["ran_cigar_lanes"] == 16
    _check(recs, lambda p: ops[p, :recs["n_ops"][p]], reads, refs, exp[True], plan[True], ("quads", form, "device"))
    _check_host(eng.align_cigar_host(host.SW, np.array(reads), np.array(refs), extended=True, threads=2), reads, refs, exp[True], plan[True],
                ("quads", form, "host"))
    eng.close()


# ---- 3. stride cuts ----
def _closed_by(runs, W):
    """per run of the (extended) plan, what stores it: "inside" -- the next boundary lies in the step it began in (`at < cap`) --,
    "carried" -- in a later step (`count - 1 < cap` in the loop) --, "end" -- the store behind the loop"""
    at = cp.boundaries(runs) + [cp.columns(runs)]
    return ["end" if e == at[-1] else "inside" if e // W == s // W else "carried" for s, e in zip(at, at[1:])]


def _cut_cases(W):
    names = ("x@%d" % (W - 2), "x@%d" % (W - 1), "x@%d" % W, "span2steps", "alternate", "I=D", "eq%d" % (2 * W + 1))
    by_name = {c.name: c for c in cp.plans(W)}
    return [by_name[k] for k in names]


@pytest.mark.parametrize("W", WIDTHS)
def test_stride_cuts(monkeypatch, W):
    """ops_stride in 1, k - 1, k, k + 1 for plans of k runs: the stored prefix is exact, n_ops the true count, every word past
    min(k, stride) of a pair and the word in front of the first pair's ops still hold the sentinel."""
    R, F = SHAPES[0]
    cases = _cut_cases(W)
    reads, refs, exp, plan = _expect(cases, R, F, "aff")
    want, want_recs = plan[True]
    strides = sorted({s for o in want for s in (1, len(o) - 1, len(o), len(o) + 1) if s >= 1})
    # the first run that is not stored is, somewhere, of each kind: the cut falls on every guard
    cut = {_closed_by(c.runs, W)[s] for c, o in zip(cases, want) for s in (1, len(o) - 1) if 1 <= s < len(o)}
    assert cut == {"inside", "carried", "end"}, cut
    eng = _engine(monkeypatch, R, F, "aff", W)
    d_reads, d_refs = _cuda(reads), _cuda(refs)
    n = len(cases)
    for stride in strides:
        buf = torch.full((n + 1, stride), SENTINEL, dtype=torch.int32, device="cuda")
        recs = torch.empty((n, 6), dtype=torch.int32, device="cuda")
        eng.align_cigar_device(host.SW, d_reads, d_refs, extended=True, ops_stride=stride, out=(recs, buf[1:]))
        torch.cuda.synchronize()
        assert eng.describe(0, n)["ran_cigar_lanes"] == W
        got = buf.cpu().numpy().view(np.uint32)
        assert (got[0] == SENTINEL).all(), (W, stride, "the words in front of the first pair's ops")
        assert np.array_equal(recs.cpu().numpy().astype(np.int64), want_recs), (W, stride, "records: n_ops is the true count")
        for p, o in enumerate(want):
            k = min(len(o), stride)
            assert got[p + 1, :k].tolist() == o[:k], (W, stride, cases[p].name, "stored prefix")
            assert (got[p + 1, k:] == SENTINEL).all(), (W, stride, cases[p].name, "words past the stored ops")
    eng.close()


# ---- 4. the backward encoder ----
@functools.lru_cache(maxsize=None)
def _span_expect(W, form):
    cases, reads, refs, exp, plan = _own_list(W, form)
    osc = cp.scoring(form, cpu_ref.Scoring.make)
    sp = span_cigar_ref.expected(reads, refs, osc, affine=cp.is_affine(form), extended=True)
    _frozen(sp["recs"], sp["rows"], sp["idx"])
    return sp


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("forced", WIDTHS)
@pytest.mark.parametrize("W", WIDTHS)
def test_the_backward_encoder(monkeypatch, W, forced, form):
    """span_cigar_encode_kernel<forced> on the plans of W: against tests/span_cigar_ref.py, against the plans, and -- planted
    alignments are unique -- against align_cigar_device of the same engine."""
    cases, reads, refs, exp, plan = _own_list(W, form)
    R, F = cp.shape(W)
    sp = _span_expect(W, form)
    hsc = cp.scoring(form, hipkernel.Scoring.make)
    assert span_cases.span_ref_length(R, F, hsc) >= max(cp.ref_bases(c.runs) for c in cases), "the window does not hold the plans"
    eng = _engine(monkeypatch, R, F, form, forced)
    assert eng.describe(0, 1)["span_ref_length"] == span_cases.span_ref_length(R, F, hsc)
    stride = _stride(plan)
    fwd_recs, fwd_ops = _device(eng, reads, refs, True, stride)
    for ext in (False, True):
        want_ops = sp["ops"] if ext else [o if hit else [] for o, hit in zip(cigar_ref.ops_of_rows(sp["rows"], sp["idx"], False), sp["ops"])]
        want_recs = sp["recs"].copy()
        want_recs[:, 5] = [len(o) for o in want_ops]
        assert want_ops == plan[ext][0] and np.array_equal(want_recs, plan[ext][1])           # the reference against the plans
        recs, ops = eng.align_span_device(host.SW, _cuda(reads), _cuda(refs), extended=ext, ops_stride=stride, out=_outputs(len(cases), stride))
        torch.cuda.synchronize()
        assert eng.describe(0, len(cases))["ran_cigar_lanes"] == forced
        recs, ops = recs.cpu().numpy().astype(np.int64), ops.cpu().numpy().view(np.uint32)
        assert np.array_equal(recs, want_recs), (W, forced, form, ext, np.nonzero((recs != want_recs).any(axis=1))[0][:8].tolist())
        for p, o in enumerate(want_ops):
            assert ops[p, :len(o)].tolist() == o, (W, forced, form, ext, cases[p].name)
        if ext:
            assert np.array_equal(recs, _as_rows(fwd_recs)), "the spanned records are align_cigar_device's"
            assert all(np.array_equal(ops[p, :recs[p, 5]], fwd_ops[p, :recs[p, 5]]) for p in range(len(cases))), "the spanned ops are align_cigar_device's"
        h_recs, h_ops, offsets = eng.align_span_host(host.SW, np.array(reads), np.array(refs), extended=ext, threads=2)
        assert eng.describe(0, len(cases))["ran_cigar_lanes"] == forced
        assert np.array_equal(_as_rows(h_recs), want_recs) and offsets[0] == 0 and np.array_equal(np.diff(offsets), want_recs[:, 5])
        assert h_ops.tolist() == [x for o in want_ops for x in o], (W, forced, form, ext, "host ops")
    eng.close()


# ---- 5. extension alignments ----
@functools.lru_cache(maxsize=None)
def _extend_expect(W, form, banded):
    """the reference's results for BONUSES, extended and not: the register route's from extend_align_ref, the banded route's
    from extend_band_align_ref under a band wider than the matrix"""
    cases, reads, refs, exp, plan = _own_list(W, form)
    R, F = cp.shape(W)
    osc = cp.scoring(form, cpu_ref.Scoring.make)
    affine = cp.is_affine(form)
    if banded:
        return {ext: ebar.align(reads, refs, osc, _band(R, F), affine, end_bonus=BONUSES, extended=ext) for ext in (False, True)}
    return {ext: ear.align(reads, refs, osc, affine, end_bonus=BONUSES, extended=ext) for ext in (False, True)}


def _band(R, F):
    return 2 * max(R, F) + 2


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("banded", [False, True])
@pytest.mark.parametrize("forced", WIDTHS)
@pytest.mark.parametrize("W", WIDTHS)
def test_extension_alignments(monkeypatch, W, forced, banded, form):
    """The plans begin at column 0 and end at both sequences' ends: from the anchor, the extension alignment to the best cell
    (end_bonus -1) and to the read end (INT32_MAX) is the plan.  The register route and the banded route (a band wider than
    the matrix), device and host entry."""
    cases, reads, refs, exp, plan = _own_list(W, form)
    R, F = cp.shape(W)
    want = _extend_expect(W, form, banded)
    planted = [k for k, c in enumerate(cases) if c.kind == "plan"]
    eng = _engine(monkeypatch, R, F, form, forced)
    if banded:
        eng.set_band_width(_band(R, F))
        eng.set_extend_band(1)
        eng.set_extend_band_align(1)
    stride = max(_stride(plan), 3)
    for ext in (False, True):
        for bonus, res in zip(BONUSES, want[ext]):
            what = (W, forced, banded, form, ext, bonus)
            want_recs, want_ops, want_ext = res[:3]
            for k in planted:                           # the reference against the plans
                assert want_ops[k] == plan[ext][0][k] and want_recs[k].tolist() == plan[ext][1][k].tolist(), (what, cases[k].name)
            recs, ops, extend = eng.align_extend_device(host.SW, _cuda(reads), _cuda(refs), end_bonus=bonus, extended=ext, ops_stride=stride,
                                                        out=_outputs(len(cases), stride, extend=True))
            torch.cuda.synchronize()
            d = eng.describe(0, len(cases))
            assert d["ran_cigar_lanes"] == forced and d["ran_extend_align"] == ("band" if banded else "rows"), (what, d["ran_extend_align"])
            recs, ops = recs.cpu().numpy().astype(np.int64), ops.cpu().numpy().view(np.uint32)
            assert np.array_equal(recs, want_recs), (what, np.nonzero((recs != want_recs).any(axis=1))[0][:8].tolist())
            assert np.array_equal(extend.cpu().numpy().astype(np.int64), want_ext), (what, "extension records")
            for p, o in enumerate(want_ops):
                k = min(len(o), stride)
                assert ops[p, :k].tolist() == o[:k], (what, cases[p].name)
            if ext:
                h_recs, h_ops, offsets, _ = eng.align_extend_host(host.SW, np.array(reads), np.array(refs), end_bonus=bonus, extended=True, threads=2)
                assert eng.describe(0, len(cases))["ran_cigar_lanes"] == forced
                assert np.array_equal(_as_rows(h_recs), want_recs) and offsets[0] == 0 and np.array_equal(np.diff(offsets), want_recs[:, 5]), what
                assert h_ops.tolist() == [x for o in want_ops for x in o], (what, "host ops")
    eng.close()


# ---- 6. the scan ----
@pytest.mark.parametrize("form", FORMS)
def test_the_scan(monkeypatch, form):
    """cigar_scan_kernel over 1023, 1024, 1025 and 2049 records (one block of 1024 threads: a partial round, a whole one, one
    pair into the second, one into the third), n_ops from 0 to 2 W + 3: offsets are the exclusive prefix sum of the plans' op
    counts, offsets[n] their total, and the emit pass puts every pair's ops there."""
    W = 16
    cases, reads, refs, exp, plan = _own_list(W, form)
    R, F = cp.shape(W)
    counts = np.array([len(o) for o in plan[True][0]], np.int64)
    assert counts.min() == 0 and counts.max() == 2 * W + 3
    eng = _engine(monkeypatch, R, F, form)
    for n in (1023, 1024, 1025, 2049):
        pick = np.arange(n) % len(cases)
        recs, ops, offsets = eng.align_cigar_host(host.SW, np.ascontiguousarray(reads[pick]), np.ascontiguousarray(refs[pick]), extended=True, threads=4)
        want = np.concatenate([[0], np.cumsum(counts[pick])])
        assert np.array_equal(offsets, want), (n, "offsets", np.nonzero(offsets != want)[0][:8].tolist())
        assert offsets[n] == counts[pick].sum() == len(ops)
        assert np.array_equal(_as_rows(recs), plan[True][1][pick]), (n, "records")
        flat = np.array([x for k in pick for x in plan[True][0][k]], np.uint32)
        assert np.array_equal(ops, flat), (n, "ops at the scanned offsets")
    eng.close()


# ---- 7. one row-strip leg ----
@pytest.mark.parametrize("forced", [None, 16])
def test_a_long_alignment(monkeypatch, forced):
    """1025 x 1200, one pair of 1025 columns: 17 steps of the engine's own 64 lanes, 65 steps of 16 -- the only place a long
    alignment meets <16>; '=' runs carried over 3, 6 and 5 whole steps of 64 (15, 27 and 20 of 16), both X on a last lane."""
    R, F = cp.STRIP_SHAPE
    case = cp.strip_case()
    reads, refs, exp, plan = _expect([case], R, F, "aff")
    eng = _engine(monkeypatch, R, F, "aff", forced)
    recs, ops = _device(eng, reads, refs, True, 8)
    d = eng.describe(0, 1)
    assert d["ran_cigar_lanes"] == (forced or 64) and d["ran_align_fill"].startswith("strip"), d
    _check(recs, lambda p: ops[p, :recs["n_ops"][p]], reads, refs, exp[True], plan[True], ("strip", forced, "device"))
    _check_host(eng.align_cigar_host(host.SW, np.array(reads), np.array(refs), extended=False, threads=1), reads, refs, exp[False], plan[False],
                ("strip", forced, "host"))
    eng.close()
