"""Every cell-format range rule walked to its edge, and both sides of the edge judged exactly.

Each score and alignment call picks its cell format (f16 / int16 / int32) and its fill kernel from closed-form bounds
(versalignlib_amd/csrc/cell_rules.h: half_float_exact, half_float_unit_exact, int16_range_ok, tagged_range_ok,
affine_tagged_range_ok, lane_key_ok, prof_key_ok, border_bad, int32_refused; score_gap_form, fill_choice and align_route choose
with them).  A bound one term too loose does not
fail: it returns a rounded half or a wrapped short for some inputs only.  So each row of ROWS walks one parameter of one
rule at a fixed shape and mode, reads what the engine REPORTS it launched (describe / the plugin's log: ran_score_cells,
ran_align_fill -- not the prediction), finds the last value that runs the narrow form and the first that does not, and
runs a batch built to reach the bound's extremes at both values against the int32 oracle (cpu_ref ..., wide=True; where
the reference's int16 would wrap, the score is the value saturated to a short).  Tiny shapes with extreme scorings are
judged by exhaustive enumeration (tests/enumerate_alignments.py), which shares no code with the oracle.
tests/cell_rules_check.cpp walks the same families over the rules alone, on the CPU, value by value: one transition each."""
import numpy as np
import pytest

import enumerate_alignments as en
from oracle import cpu_ref
from versalignlib_amd import build, hipkernel, host, synth

pytestmark = pytest.mark.gpu

SW, NW = host.SW, host.NW


def S(m=2, mm=-1, gr=-3, gf=None, aff=None):
    """scoring: match, mismatch, linear gaps (gap_ref defaults to gap_read), aff = (open_read, ext_read, open_ref, ext_ref)"""
    gf = gr if gf is None else gf
    return dict(m=m, mm=mm, gr=gr, gf=gf, aff=aff)


def _args(s):
    """Scoring.make arguments: the opening / extension scores only for affine gaps (they make the scoring affine)"""
    return (s["m"], s["mm"], s["gr"], s["gf"]) + tuple(s["aff"] or ())


def _keys(s):
    k = dict(score_match=s["m"], score_mismatch=s["mm"], score_gap_read=s["gr"], score_gap_ref=s["gf"])
    if s["aff"]:
        k.update(zip(("score_gap_open_read", "score_gap_extend_read", "score_gap_open_ref", "score_gap_extend_ref"), s["aff"]))
    return k


def edge_batch(R, F, n, seed):
    """Pairs that reach the bounds' extremes: identical prefixes (SW reaches min(R, F) * match in the last row, the
    largest row bits of the lane key), all-mismatch pairs (the NW lower bounds), one long deletion / insertion (E / F
    runs, the NW tilt), the read repeated inside the reference (tied maxima, the first-maximum rule), and synth's N runs,
    junk bytes, lower case and NUL-padded short pairs."""
    reads, refs = synth.make_pairs(n, R, F, seed=seed, sub_rate=0.05, n_run_frac=0.1, short_frac=0.1, lowercase_frac=0.05, junk_frac=0.05)
    rng = np.random.default_rng(seed)
    m, q = min(R, F), max(1, n // 6)
    for p in range(n):
        kind = p // q
        if kind == 0:                                   # identical
            reads[p, :m] = refs[p, :m]
        elif kind == 1:                                 # all mismatch
            reads[p] = ord("A")
            refs[p] = ord("C")
        elif kind == 2:                                 # one long deletion from the read / insertion into it
            k = max(2, m // 4)
            a = int(rng.integers(1, max(2, m - k)))
            if p % 2 and R + k <= F:                    # the read skips k reference bases
                reads[p] = np.concatenate([refs[p, :a], refs[p, a + k:R + k]])
            else:                                       # the read carries k bases the reference does not
                src = np.concatenate([refs[p, :a], np.full(k, ord("T"), np.uint8), refs[p, a:]])
                reads[p, :min(R, src.size)] = src[:R]
        elif kind == 3 and 2 * R <= F:                  # the read twice in the reference
            refs[p, :R] = reads[p]
            refs[p, R:2 * R] = reads[p]
    return np.ascontiguousarray(reads), np.ascontiguousarray(refs)


# ---- one call of a row's kind at one scoring -> (result, what ran) ----

def _engine(row, s, R, F):
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*_args(s)), group_lanes=row.get("G", 0), rows_per_lane=row.get("K", 0))
    if row.get("sse"):
        eng.set_traceback_policy(1)
    return eng


def run_call(row, s, reads, refs):
    import torch
    opt, kind = row["opt"], row["kind"]
    R, F = reads.shape[1], refs.shape[1]
    if row.get("api") == "plugin":
        keys = _keys(s)
        if row.get("sse"):
            keys["traceback_policy"] = 1
        with host.Plugin(build.HIP_PLUGIN, R, F, num_threads=4, **keys) as hip:
            hip.drain_log()
            got = hip.score_alignments(opt, reads, refs) if kind == "score" else hip.compute_alignments(opt, reads, refs)
            ran = hip.last_ran()
        return got, ran["ran_score_cells" if kind == "score" else "ran_align_fill"]
    eng = _engine(row, s, R, F)
    try:
        d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
        if kind == "score":
            got = eng.score_device(opt, d_reads, d_refs).cpu().numpy()
        else:
            r, i = eng.align_device(opt, d_reads, d_refs)
            got = (r.cpu().numpy(), i.cpu().numpy())
        d = eng.describe(opt)
        return got, d["ran_score_cells" if kind == "score" else "ran_align_fill"]
    finally:
        eng.close()


def oracle(row, s, reads, refs):
    osc = cpu_ref.Scoring.make(*_args(s))
    aff = s["aff"] is not None
    if row["kind"] == "score":
        return cpu_ref.score(row["opt"], reads, refs, osc, threads=8, affine=aff, wide=True)
    kw = dict(affine=True) if aff else dict(policy="sse" if row.get("sse") else "default")
    return cpu_ref.align(row["opt"], reads, refs, osc, threads=8, wide=True, **kw)


def same(got, exp):
    if isinstance(got, tuple):
        return np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    return np.array_equal(got, exp)


def R_(rule, kind, opt, R, F, lo, hi, scoring, narrow, n=240, **kw):
    return dict(id="%s-%s" % (rule, "sw" if opt == SW else "nw"), kind=kind, opt=opt, R=R, F=F, lo=lo, hi=hi, sc=scoring,
                narrow=narrow, n=n, **kw)


AFF20 = (-20, -3, -20, -3)
NOT_INT32 = ("f16", "int16")
NOT_WIDE = ("fused_tag", "tag_prof_key", "tag_key", "tag", "sse_tag_key", "sse_tag", "sse", "affine_tag_sym", "affine_tag",
            "affine_sym", "affine", "linear_sym", "linear", "strip")

# Each row: rule, kind, mode, shape, the walked range (narrow at lo, not at hi), the scoring at a walked value, what counts as
# the narrow form.  Walked values are magnitudes where the parameter is a penalty.
ROWS = [
    # half_float_exact: affine score cells, SW; NW on the small-call (latency) plan and on the large-call plan
    R_("half_float_exact", "score", SW, 150, 500, 1, 30, lambda v: S(v, -11, -20, aff=AFF20), ("f16",)),
    R_("half_float_exact_small_call", "score", NW, 150, 500, 1, 30, lambda v: S(v, -11, -20, aff=AFF20), ("f16",)),
    R_("half_float_exact_large_call", "score", NW, 150, 500, 1, 30, lambda v: S(v, -11, -20, aff=AFF20), ("f16",), tile=100),
    # ... linear NW: the tilted frame's span grows with the gap score
    R_("half_float_exact_linear", "score", NW, 150, 500, 1, 20, lambda v: S(2, -1, -v), ("f16",)),
    R_("half_float_exact_mismatch", "score", NW, 150, 500, 50, 700, lambda v: S(2, -v, -1), ("f16",)),
    # ... NW slack <= 512, which binds where nothing else does: free gaps, a small top (50 x 100, match 1)
    R_("half_float_exact_slack", "score", NW, 50, 100, 400, 600, lambda v: S(1, -v, 0), ("f16",)),
    # half_float_unit_exact: linear SW on the register kernels and on the long strips
    R_("half_float_unit_exact", "score", SW, 150, 500, 1, 12, lambda v: S(v, -1, -3), ("f16",)),
    R_("half_float_unit_exact_slack", "score", SW, 150, 500, 100, 600, lambda v: S(2, -v, -3), ("f16",)),
    R_("half_float_unit_exact_long", "score", SW, 150, 8000, 1, 12, lambda v: S(v, -1, -3), ("f16",), n=24),
    # int16_range_ok: scores (int16 or f16 vs int32 strips), alignments (anything vs the int32 strips)
    R_("int16_range_score", "score", SW, 150, 500, 150, 300, lambda v: S(v, -1, -3), NOT_INT32),
    R_("int16_range_score_abi", "score", SW, 150, 500, 150, 300, lambda v: S(v, -1, -3), NOT_INT32, api="plugin"),
    # ... by read length at match 200: hi = 200 R + 1 > 32000 from R = 160, one unit of the bound visible
    R_("int16_range_read_length", "score", SW, 150, 500, 140, 180, lambda v: S(200, -1, -3), NOT_INT32, shape=lambda v: (v, 500)),
    R_("int16_range_score", "score", NW, 150, 500, 150, 300, lambda v: S(2, -v, -1), NOT_INT32),
    R_("int16_range_score_abi", "score", NW, 150, 500, 150, 300, lambda v: S(2, -v, -1), NOT_INT32, api="plugin"),
    R_("int16_range_score_affine_nw_lo", "score", NW, 150, 500, 60, 200, lambda v: S(2, -v, -5, aff=(-5, -1, -5, -1)), NOT_INT32),
    R_("int16_range_align", "align", SW, 150, 500, 150, 300, lambda v: S(v, -1, -3), NOT_WIDE),
    R_("int16_range_align_abi", "align", SW, 150, 500, 150, 300, lambda v: S(v, -1, -3), NOT_WIDE, api="plugin"),
    R_("int16_range_align", "align", NW, 150, 500, 150, 300, lambda v: S(2, -v, -1), NOT_WIDE),
    R_("int16_range_align_abi", "align", NW, 150, 500, 150, 300, lambda v: S(2, -v, -1), NOT_WIDE, api="plugin"),
    R_("int16_range_align_affine_nw_lo", "align", NW, 150, 500, 60, 200, lambda v: S(2, -1, -v, aff=(-v, -v, -v, -v)), NOT_WIDE),
    # border_bad: column 0 of the NW variant, a gap of the whole read (binds where the reference is the short side)
    R_("border_bad", "align", NW, 400, 50, 40, 120, lambda v: S(2, -1, -1, -v), NOT_WIDE),
    # tagged_range_ok (4 x range, 2-bit tag) and the SW keys: prof_key_ok, lane_key_ok (4 bits), plain tags
    R_("prof_key", "align", SW, 150, 500, 1, 20, lambda v: S(v, -1, -3), ("tag_prof_key",)),
    R_("prof_key_mismatch", "align", SW, 150, 500, 200, 300, lambda v: S(1, -v, -3), ("tag_prof_key",)),
    R_("prof_key_gap", "align", SW, 150, 500, 450, 550, lambda v: S(1, -1, -v), ("tag_prof_key",)),
    R_("lane_key", "align", SW, 150, 500, 1, 40, lambda v: S(v, -1, -3), ("tag_prof_key", "tag_key")),
    R_("lane_key_5bit", "align", SW, 150, 500, 1, 40, lambda v: S(v, -1, -3), ("tag_key",), G=64, K=32),
    R_("tagged", "align", SW, 150, 500, 20, 100, lambda v: S(v, -1, -3), ("tag_prof_key", "tag_key", "tag")),
    R_("tagged", "align", NW, 150, 500, 20, 100, lambda v: S(v, -1, -1), ("tag",)),
    R_("tagged_mismatch", "align", SW, 150, 500, 1900, 2100, lambda v: S(1, -v, -3), ("tag_key",)),
    R_("tagged_lo_gap", "align", SW, 150, 500, 7900, 8100, lambda v: S(1, -1, -v), ("tag_key",)),
    R_("tagged_lo", "align", NW, 150, 500, 2, 40, lambda v: S(2, -v, -1, -1), ("tag",)),
    R_("sse_lane_key", "align", SW, 150, 500, 1, 40, lambda v: S(v, -1, -3), ("sse_tag_key",), sse=True),
    R_("sse_tagged", "align", SW, 150, 500, 20, 100, lambda v: S(v, -1, -3), ("sse_tag_key", "sse_tag"), sse=True),
    R_("sse_tagged", "align", NW, 150, 500, 2, 40, lambda v: S(2, -v, -1), ("sse_tag",), sse=True),
    # affine_tagged_range_ok (8 x range): SW lane key, NW lower bound 8 lo - 8 >= -28000
    R_("affine_tagged", "align", SW, 150, 500, 1, 40, lambda v: S(v, -1, -5, aff=(-5, -1, -5, -1)), ("affine_tag_sym",)),
    R_("affine_tagged_asym", "align", SW, 150, 500, 1, 40, lambda v: S(v, -1, -5, aff=(-5, -1, -6, -2)), ("affine_tag",)),
    R_("affine_tagged_lo", "align", NW, 150, 500, 100, 900, lambda v: S(2, -1, -v, aff=(-v, -1, -v, -1)), ("affine_tag_sym",)),
    # ... NW upper bound 8 hi + 8 <= 32000 (hi = 150 match + 1 + 161 rows of tilt + 501 columns): by match, then by ref_length
    # at match 22, where one unit of the bound is one column
    R_("affine_tagged_hi", "align", NW, 150, 500, 2, 40, lambda v: S(v, -1, -5, aff=(-5, -1, -5, -1)), ("affine_tag_sym",)),
    R_("affine_tagged_hi_ref_length", "align", NW, 150, 500, 500, 600, lambda v: S(22, -1, -5, aff=(-5, -1, -5, -1)), ("affine_tag_sym",),
       shape=lambda v: (150, v)),
    # ... NW row tilt |ext_ref| (rows + 1) <= 3500: binds before the lower bound only where the sweep's rows outnumber
    # R + F (a forced 64 x 8 geometry, 9 x 5 pairs: 513 |ext_ref| against 16 |ext_ref|)
    R_("affine_tagged_tilt", "align", NW, 9, 5, 2, 20, lambda v: S(1, -1, -1, -v, aff=(-1, -1, -v, -v)), ("affine_tag",), G=64, K=8),
    # ... SW 5-bit key for more than 16 rows per lane (full 64 x 32 geometry: it carries the affine-tagged fills)
    R_("affine_tagged_5bit", "align", SW, 150, 500, 1, 40, lambda v: S(v, -1, -5, aff=(-5, -1, -5, -1)), ("affine_tag_sym",), G=64, K=32),
    # ... |mismatch| < 1000 (SW: the lower bound is one mismatch, 8 lo - 8 >= -28000 allows 3 499)
    R_("affine_tagged_mismatch", "align", SW, 150, 500, 900, 1100, lambda v: S(2, -v, -5, aff=(-5, -1, -5, -1)), ("affine_tag_sym",)),
    # the fused small-call kernel (align_route: Fused) on both sides of tagged_range_ok(alg, 256): 1 000 pairs of 64 x 128 through the ABI
    R_("fused", "align", SW, 64, 128, 60, 200, lambda v: S(v, -1, -3), ("fused_tag",), n=1000, api="plugin"),
    R_("fused", "align", NW, 64, 128, 60, 200, lambda v: S(v, -1, -1), ("fused_tag",), n=1000, api="plugin"),
]


# The transitions each rule puts at its row's shape (last narrow value, first other one), worked out from the bound:
# a rule whose edge moves -- loosened or tightened by one unit where the shape makes that unit visible -- fails its row.
#
# Clauses (of the rules in cell_rules.h, by function name) with no row, and why:
#   unreachable -- implied by a stricter clause of the same rule for every input:
#     half_float_exact SW  slack <= 1024          (top + 2 slack <= 2048, top >= 0)
#     half_float_exact NW  span < 30000           (centre + 3 slack <= 2048 keeps span <= 4096)
#     half_float_unit_exact  slack < 512          (top + 2 slack < 1024)
#     affine_tagged_range_ok SW  8 hi + 8 <= 32000 (its own lane-key clause (hi + 1) << 4 binds first)
#     affine_tagged_range_ok NW  |ext_read| (F + 1) <= 3500  (the lower bound's (R + F + 2) |ext| binds first)
#   reachable, not walked -- they bind only at shapes of at most a few rows:
#     tagged_range_ok |match| < 2000 (min(R, F) <= 3), affine_tagged_range_ok |match| < 1000 (min(R, F) <= 1 for SW,
#     <= 3 for NW)
#   walked, but one unit of the bound is no visible step at any shape:
#     affine_tagged_range_ok NW row tilt: 3 501 is no multiple of a geometry's rows + 1
EDGES = {
    "half_float_exact-sw": (13, 14),
    "half_float_exact_small_call-nw": (11, 12),
    "half_float_exact_large_call-nw": (13, 14),
    "half_float_exact_linear-nw": (4, 5),
    "half_float_exact_mismatch-nw": (210, 211),
    "half_float_unit_exact-sw": (6, 7),
    "half_float_unit_exact_slack-sw": (361, 362),
    "half_float_unit_exact_long-sw": (6, 7),
    "int16_range_score-sw": (213, 214),
    "int16_range_score_abi-sw": (213, 214),
    "int16_range_score-nw": (210, 211),
    "int16_range_score_abi-nw": (210, 211),
    "int16_range_score_affine_nw_lo-nw": (98, 99),
    "int16_range_align-sw": (213, 214),
    "int16_range_align_abi-sw": (213, 214),
    "int16_range_align-nw": (210, 211),
    "int16_range_align_abi-nw": (210, 211),
    "int16_range_align_affine_nw_lo-nw": (98, 99),
    "border_bad-nw": (79, 80),
    "prof_key-sw": (3, 4),
    "prof_key_mismatch-sw": (249, 250),
    "prof_key_gap-sw": (499, 500),
    "lane_key-sw": (13, 14),
    "lane_key_5bit-sw": (6, 7),
    "tagged-sw": (53, 54),
    "tagged-nw": (48, 49),
    "tagged_lo-nw": (12, 13),
    "sse_lane_key-sw": (13, 14),
    "sse_tagged-sw": (53, 54),
    "sse_tagged-nw": (12, 13),
    "affine_tagged-sw": (13, 14),
    "affine_tagged_asym-sw": (13, 14),
    "affine_tagged_lo-nw": (569, 570),
    "affine_tagged_hi-nw": (22, 23),
    "affine_tagged_hi_ref_length-nw": (536, 537),
    "affine_tagged_tilt-nw": (6, 7),
    "affine_tagged_5bit-sw": (6, 7),
    "affine_tagged_mismatch-sw": (999, 1000),
    "tagged_mismatch-sw": (1999, 2000),
    "tagged_lo_gap-sw": (7999, 8000),
    "half_float_exact_slack-nw": (512, 513),
    "int16_range_read_length-sw": (159, 160),
    "fused-sw": (124, 125),
    "fused-nw": (118, 119),
}


def _walk(row, batch):
    """-> (last narrow value, what it ran, first other value, what that ran); bisection over [lo, hi] after checking
    both ends, so a changed rule cannot leave the row without a transition.  batch(v): the pairs at walked value v."""
    ran = {}

    def probe(v):
        if v not in ran:
            ran[v] = run_call(row, row["sc"](v), *batch(v))[1]
        return ran[v] in row["narrow"]

    lo, hi = row["lo"], row["hi"]
    assert probe(lo), "%s: %d does not run the narrow form (%s)" % (row["id"], lo, ran[lo])
    assert not probe(hi), "%s: %d still runs the narrow form (%s): no transition inside the walk" % (row["id"], hi, ran[hi])
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if probe(mid):
            lo = mid
        else:
            hi = mid
    return lo, ran[lo], hi, ran[hi]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r["id"])
def test_range_edge(row):
    batches = {}

    def batch(v):                                   # (rows that walk the shape: a batch per shape)
        R, F = row["shape"](v) if "shape" in row else (row["R"], row["F"])
        if (R, F) not in batches:
            reads, refs = edge_batch(R, F, row["n"], seed=row["R"] * 7 + row["F"] + row["opt"])
            if row.get("tile"):                     # a large call: the engine's own plan instead of the latency plan
                reads, refs = np.tile(reads, (row["tile"], 1)), np.tile(refs, (row["tile"], 1))
            batches[(R, F)] = reads, refs
        return batches[(R, F)]

    a, ran_a, b, ran_b = _walk(row, batch)
    print("%s: narrow (%s) up to %d, %s from %d" % (row["id"], ran_a, a, ran_b, b))
    assert (a, b) == EDGES[row["id"]], "%s: the edge moved from %r to %r" % (row["id"], EDGES[row["id"]], (a, b))
    n = row["n"]
    for v in (a, b):
        s = row["sc"](v)
        reads, refs = batch(v)
        R, F = reads.shape[1], refs.shape[1]
        got, ran = run_call(row, s, reads, refs)
        exp = oracle(row, s, reads[:n], refs[:n])
        head = (got[0][:n], got[1][:n]) if isinstance(got, tuple) else got[:n]
        assert same(head, exp), "%s at %d (%s): differs from the oracle" % (row["id"], v, ran)
        if row.get("tile"):                         # every copy of the batch gives the same answer
            if isinstance(got, tuple):
                assert all(np.array_equal(g.reshape((row["tile"],) + h.shape), np.broadcast_to(h, (row["tile"],) + h.shape)) for g, h in zip(got, head))
            else:
                assert np.array_equal(got.reshape(row["tile"], n), np.broadcast_to(head, (row["tile"], n)))
        if row["kind"] == "score" and exp.size:
            # the batch reaches the bound: the identical pairs score min(R, F) * match (saturated) in SW
            if row["opt"] == SW and s["m"] > 0 and F >= R:
                assert exp.max() == min(32767, min(R, F) * s["m"])


def test_small_calls_report_the_latency_plan_format():
    """describe(opt, n) predicts with the plan a device call of n pairs launches; after the call the engine reports what it
    launched -- the two agree on both sides of the NW half-float edge for a small and a large call."""
    import torch
    R, F = 150, 500
    reads, refs = edge_batch(R, F, 240, seed=5)
    for n_tile in (1, 100):
        rd, rf = np.tile(reads, (n_tile, 1)), np.tile(refs, (n_tile, 1))
        d_reads, d_refs = torch.from_numpy(rd).cuda(), torch.from_numpy(rf).cuda()
        for match in range(1, 30):
            eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(match, -11, -20, -20, *AFF20))
            predicted = eng.describe(NW, rd.shape[0])["score_cells"]
            eng.score_device(NW, d_reads, d_refs)
            torch.cuda.synchronize()
            assert eng.describe(NW)["ran_score_cells"] == predicted, (n_tile, match)
            eng.close()


@pytest.mark.parametrize("opt", [SW, NW])
def test_int32_refusal_edge(opt):
    """(R + F + 2) * |score| >= 2^28 is refused with a message; one unit below, the int32 strips answer exactly."""
    R, F = 100, 8092                                 # R + F + 2 = 8194: refused from |score| 32761 on
    reads, refs = edge_batch(R, F, 4, seed=11)
    reads[0] = refs[0, :R]
    row = dict(kind="align", opt=opt, R=R, F=F)
    ok = S(32760, -1, -3)
    got, ran = run_call(row, ok, reads, refs)
    print("int32 refusal: %d runs on %s" % (32760, ran))
    assert ran == "strip_wide"
    assert same(got, oracle(row, ok, reads, refs))
    with pytest.raises(hipkernel.HipKernelError, match="int32 range"):
        run_call(row, S(32761, -1, -3), reads, refs)
    with host.Plugin(build.HIP_PLUGIN, R, F, **_keys(S(32761, -1, -3))) as hip:
        with pytest.raises(host.PluginError, match="int32 range"):
            hip.compute_alignments(opt, reads, refs)
        assert hip.last_ran() is None


TINY = [
    (3, 3, S(12000, -1, -1)), (3, 5, S(12000, -32768, -32768)), (6, 6, S(32767, -32768, -32768, -1)),
    (5, 4, S(1, -32768, -1, -32768)), (4, 6, S(9000, -4000, -30000, aff=(-30000, -100, -2, -2))),
    (6, 3, S(20000, -20000, -32768, aff=(-32768, -1, -32768, -1))), (2, 6, S(32767, -1, -5, aff=(-5, -5, -32768, -32767))),
]


@pytest.mark.parametrize("R,F,s", TINY, ids=["%dx%d-%d" % (R, F, k) for k, (R, F, _) in enumerate(TINY)])
def test_tiny_shapes_extreme_scorings_against_enumeration(R, F, s):
    """Shapes of at most 6 x 6 with scorings far outside int16, judged by walking every alignment: scores (saturated to
    a short) and alignments that end in the enumerated end cell and re-score to its value."""
    import torch
    pairs = [(b"ACGTAC", b"ACGTAC"), (b"AAAAAA", b"CCCCCC"), (b"ACGTTG", b"ACTTGA"), (b"GAGAGA", b"AGAGAG"),
             (b"ANNCAT", b"AGTCAT"), (b"AC\xffGTT", b"ACTGTT"), (b"AC\0\0\0\0", b"ACG\0\0\0"), (b"TTTTTT", b"TGTTTT")]
    reads = np.array([np.frombuffer(a[:R], np.uint8) for a, _ in pairs])
    refs = np.array([np.frombuffer(b[:F].ljust(F, b"T"), np.uint8) for _, b in pairs])
    sc = (s["m"], s["mm"]) + tuple(s["aff"] or (s["gr"], s["gr"], s["gf"], s["gf"]))
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*_args(s)))
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    AL = R + F
    for opt in (SW, NW):
        got = eng.score_device(opt, d_reads, d_refs).cpu().numpy()
        rows, idx = (t.cpu().numpy() for t in eng.align_device(opt, d_reads, d_refs))
        d = eng.describe(opt)
        print("%dx%d %r opt %d: %s / %s" % (R, F, sc, opt, d["ran_score_cells"], d["ran_align_fill"]))
        for p in range(len(pairs)):
            read, ref = reads[p], refs[p]
            start = int(idx[p, 0])
            a, b = bytes(rows[p, 0, start:AL - 1]), bytes(rows[p, 1, start:AL - 1])
            if opt == SW:
                best = en.sw_score(read, ref, sc)
                assert got[p] == min(best, 32767), (p, opt)
                if best > 0:
                    assert en.rescore_rows(a, b, sc) == best, (p, a, b)
            else:
                assert got[p] == min(en.nw_variant_score(read, ref, sc), 32767), (p, opt)
                cells = en.nw_variant_align_cells(read, ref, sc)
                ei, ej = en.nw_variant_end_cell(read, ref, cells)
                assert en.ungapped(a) == bytes(read[:ei + 1]), (p, a, b)
                assert en.rescore_rows(a, b, sc) == cells[(ei + 1, ej + 1)], (p, a, b)
    eng.close()
