"""tests/cigar_plans.py against the oracle, without a GPU: EVERY plan of both lane widths and both scorings is the oracle's
Smith-Waterman alignment of the pair build() makes for it -- ops (extended and not), coordinates and score, which the plan
fixes by construction -- and stays that under the other tie-break policy and for the reversed pair (what the spanned CIGARs
align): planted alignments are unique, not merely first.  The lists must also hold every edge of the encoder they are there
for; that is computed from the plans, so an edit of the lists cannot lose one unnoticed."""
import functools
import random

import numpy as np
import pytest

import cigar_plans as cp
import cigar_ref
import span_cigar_ref
from oracle import cpu_ref
from versalignlib_amd import host

WIDTHS = (16, 64)
FORMS = ("lin", "aff")


@functools.lru_cache(maxsize=None)
def _oracle(W, form):
    cases = cp.for_form(cp.plans(W), form)
    R, F = cp.shape(W)
    reads, refs = cp.batch(cases, R, F)
    osc = cp.scoring(form, cpu_ref.Scoring.make)
    rows, idx = cpu_ref.align(host.SW, reads, refs, osc, threads=4, affine=cp.is_affine(form))
    for a in (reads, refs, rows, idx):
        a.setflags(write=False)
    return cases, reads, refs, osc, rows, idx


def _text(ops):
    return cigar_ref.text_of_ops(ops)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("W", WIDTHS)
def test_every_plan_is_the_oracles_alignment(W, form):
    cases, reads, refs, osc, rows, idx = _oracle(W, form)
    ends = cigar_ref.end_cells_sw(reads, refs, osc, cp.is_affine(form))
    for extended in (True, False):
        exp = cigar_ref.expected(rows, idx, osc, reads, refs, extended=extended, affine=cp.is_affine(form), ends=ends)
        for k, c in enumerate(cases):
            assert exp["ops"][k] == cp.ops(c.runs, extended), (W, form, c.name, extended, exp["text"][k], _text(cp.ops(c.runs, extended)))
            got = tuple(int(x) for x in exp["coords"][k]) + (int(exp["score"][k]), int(exp["n_ops"][k]))
            assert got == cp.record(c, form, extended), (W, form, c.name, extended, got, cp.record(c, form, extended))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("W", WIDTHS)
def test_planted_alignments_are_unique_not_first(W, form):
    """The SSE tie-break policy and the alignment of the reversed prefixes (tests/span_cigar_ref.py: ties go the other way) find
    the same ops and the same coordinates."""
    cases, reads, refs, osc, rows, idx = _oracle(W, form)
    want = [cp.ops(c.runs) for c in cases]
    rows2, idx2 = cpu_ref.align(host.SW, reads, refs, osc, threads=4, affine=cp.is_affine(form), policy="sse")
    got = cigar_ref.ops_of_rows(rows2, idx2, extended=True)
    sse = [k for k, c in enumerate(cases) if not c.n_at]           # (that policy's walk stops at a column of N: another alignment, not another tie-break)
    assert [got[k] for k in sse] == [want[k] for k in sse], [cases[k].name for k in sse if got[k] != want[k]]
    exp = span_cigar_ref.expected(reads, refs, osc, affine=cp.is_affine(form), extended=True)
    assert exp["ops"] == want, [c.name for c, a, b in zip(cases, exp["ops"], want) if a != b]
    assert exp["recs"].tolist() == [list(cp.record(c, form)) for c in cases]


@pytest.mark.parametrize("form", FORMS)
def test_the_strip_plan(form):
    """the one long plan (1025 x 1200: a row-strip shape) is the oracle's alignment too"""
    c = cp.strip_case()
    R, F = cp.STRIP_SHAPE
    reads, refs = cp.batch([c], R, F)
    osc = cp.scoring(form, cpu_ref.Scoring.make)
    rows, idx = cpu_ref.align(host.SW, reads, refs, osc, threads=1, affine=cp.is_affine(form))
    assert cigar_ref.ops_of_rows(rows, idx, extended=True) == [cp.ops(c.runs)]
    assert cigar_ref.ops_of_rows(rows, idx) == [cp.ops(c.runs, False)]
    assert int(cigar_ref.band_align_ref.rescore(rows, idx, osc, affine=cp.is_affine(form))[0]) == cp.score(c, form)
    at = cp.boundaries(c.runs)
    assert max(b - a for a, b in zip(at, at[1:] + [cp.columns(c.runs)])) > 3 * 64 and any(q % 64 == 63 for q in at)
    assert (cp.columns(c.runs) + 15) // 16 == 65


@pytest.mark.parametrize("W", WIDTHS)
def test_the_lists_hold_every_edge(W):
    cases = cp.plans(W)
    edges = cp.edges(cases, W)
    for name, held in edges.items():
        assert held, (W, name, "no plan holds this edge")
    cols = {cp.columns(c.runs) for c in cases}
    assert {0, 1, W - 1, W, W + 1, 2 * W, 2 * W + 1, 3 * W - 1, 2 * W + 3} <= cols
    # one X at column q: each boundary lane of the issue's list, by its own plan
    singles = {cp.boundaries(c.runs)[1] for c in cases if [op for _, op in c.runs] == ["=", "X", "="] and c.runs[1][0] == 1}
    assert {W - 2, W - 1, W, W + 1, 2 * W - 1, 2 * W} <= singles
    # gap runs of every listed length, of both kinds, under the affine scoring; of 1 .. 8 under the linear one
    for op in "ID":
        assert {1, W - 1, W, 2 * W + 1} <= {length for c in cases if "aff" in c.forms for length, o in c.runs if o == op}
        lin = {length for c in cases if "lin" in c.forms for length, o in c.runs if o == op}
        assert {1, cp.LINEAR_GAP_MAX} <= lin and max(lin) <= cp.LINEAR_GAP_MAX
        # ... beginning on the last lane (lane 0 extends: prev = carry_op) and on lane 0 (lane 0 opens)
        starts = {(cp.boundaries(c.runs)[1] % W, length > 1) for c in cases for length, o in c.runs[1:2] if o == op}
        assert {(W - 1, True), (0, True), (0, False)} <= starts
    assert any(c.lower_read and c.lower_ref and c.n_at for c in cases)
    assert {c.kind for c in cases} == {"plan", "noshare", "nul"}
    assert all(c.pins for c in cases)
    # the shape is the engine's own choice of this width
    R, F = cp.shape(W)
    assert (min(R, F) <= 256) == (W == 16)
    assert all(cp.read_bases(c.runs) <= R and cp.ref_bases(c.runs) <= F for c in cases)


def test_edges_are_computed_not_declared():
    """edges() on plans whose edges are known"""
    W = 16
    one = lambda runs: cp.edges([cp.Case("c", "p", tuple(runs), ("lin",), (), (), (), "plan")], W)
    held = lambda runs: {k for k, v in one(runs).items() if v}
    assert held([(W, "=")]) == set()
    assert held([(W + 1, "=")]) == {"quiet_step"}
    assert held([(W - 1, "="), (1, "X"), (1, "=")]) == {"last_lane", "lane0"}
    assert held([(1, "="), (1, "X")] * (W // 2) + [(1, "=")]) == {"full_step", "last_lane", "lane0"}
    assert held([(4 * W, "=")]) == {"quiet_step", "carried_2"}
    assert held([(3 * W - 1, "=")]) == {"quiet_step"}


def test_build_refuses_what_it_cannot_make_unique():
    rng = random.Random(1)
    for plan in ([(4, "X"), (9, "=")], [(9, "="), (2, "I")], [(9, "="), (2, "I"), (2, "D"), (9, "=")], [(9, "="), (1, "X"), (1, "I"), (9, "=")],
                 [(9, "="), (cp.MAX_X_RUN + 1, "X"), (9, "=")], [(2, "="), (1, "I"), (9, "=")], [(9, "="), (40, "D"), (9, "=")]):
        with pytest.raises(AssertionError):
            cp.build(plan, 100, 100, rng)
    with pytest.raises(AssertionError):
        cp.build([(101, "=")], 100, 200, rng)


def test_build_keeps_its_own_rules():
    """neighbouring bases differ, the junction bases of every gap run differ, X columns differ -- on every pair of both lists"""
    for W in WIDTHS:
        R, F = cp.shape(W)
        for c in cp.plans(W):
            if c.kind != "plan":
                continue
            read, ref = cp.build_case(c, R, F, random.Random(c.name))
            a, b = bytes(read).rstrip(b"\0").upper(), bytes(ref).rstrip(b"\0").upper()
            assert len(a) == cp.read_bases(c.runs) and len(b) == cp.ref_bases(c.runs)
            assert all(x != y for x, y in zip(a, a[1:])) and all(x != y for x, y in zip(b, b[1:])), c.name
            i = j = 0
            for length, op in c.runs:
                if op == "X":
                    assert all(a[i + k] != b[j + k] for k in range(length)), c.name
                elif op == "=":
                    assert a[i:i + length] == b[j:j + length], c.name
                elif op == "I":
                    assert a[i] != b[j] and a[i + length - 1] != b[j - 1], c.name          # first vs the base behind, last vs the base in front
                else:
                    assert b[j] != a[i] and b[j + length - 1] != a[i - 1], c.name
                i += length if op != "D" else 0
                j += length if op != "I" else 0
