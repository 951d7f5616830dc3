"""Every score_placed_kernel instance of libHIPKernel.so -- 68: placed_kernel<G, K, FULL> of placed_kernels.hip.h -- launched
through valign_hip_score_placed_device on its own forced geometry and compared, all three record fields, with
tests/placed_ref.py (numpy, int64 cells, independent of the library).

Each of the 17 geometries of tests/instance_matrix.py is forced at its four shapes, on both tracks (the key track where
K <= 16) and with the four gap forms.  The key track runs at match 2, the rows track at the smallest match beyond the key's
range at that shape and K.  The batches (tests/placed_matrix_cases.py; tests/test_instance_matrix_table.py holds them against
their conditions on the CPU) mix random related pairs, rotated and trimmed so that end rows and padding rows fall everywhere in
the register, with planted two-cell ties on the rows where the lane key, the row un-mapping and the first-arg-max order could go
wrong: the ends of a lane, two neighbouring lanes, the first and the last row.  The planted pairs' records are also asserted from
their construction, independently of any fill.

Which instance ran is read from describe(): ran_placed (the track) and ran_placed_geometry, set where the kernel pointer is
taken.  A geometry that does not carry the (track, form) asked for re-plans onto a full one (Engine::placed_plan_for) and asks the
rule again there: such a run must say so, must still be exact, and proves nothing about the forced geometry.  Per geometry the
instances seen must be exactly instance_matrix.carried_placed.

The re-plans of the suboptimal and the extension scores from the eleven geometries that carry none of their kernels, and the
placed re-plan at the edge of the key's range -- where the forced geometry's K and the fallback's K answer the rule differently --
are the last three tests."""
import functools

import numpy as np
import pytest
import torch

import extend_ref
import instance_matrix as im
import placed_matrix_cases as pm
import placed_ref
import subopt_ref
import test_gpu_extend as te
import test_gpu_placed as tp
import test_gpu_subopt as ts
from versalignlib_amd import hipkernel, synth

pytestmark = pytest.mark.gpu

GEOMS = sorted(im.GEOMETRIES)
LEGS = [case + (track,) for case in pm.CASES for track in pm.tracks(case[1])]
NOT_FULL = [g for g in GEOMS if not im.GEOMETRIES[g]]


def _geom_id(g):
    return "%dx%d" % g


def _leg_id(leg):
    return "%dx%d-%dx%d-%s" % leg


def _geometry(name):
    """describe()'s "GxK" -> (G, K); None for anything else"""
    parts = name.split("x")
    return tuple(int(v) for v in parts) if len(parts) == 2 and all(p.isdigit() for p in parts) else None


def _replanned_onto(name, forced, R):
    """a full geometry of the matrix other than the forced one, with at least R rows"""
    g = _geometry(name)
    return g if g is not None and im.GEOMETRIES.get(g, False) and g != forced and g[0] * g[1] >= R else None


def test_forms_are_the_placed_tests():
    assert pm.FORMS == tp.FORMS == ts.FORMS == te.FORMS and pm.PAIR_ARGS == dict(
        sub_rate=0.1, indel_rate=0.02, n_run_frac=0.1, short_frac=0.1, lowercase_frac=0.05, junk_frac=0.04)
    for R, F, K in ((150, 500, 10), (32, 7, 4), (2048, 135, 32)):
        assert pm.rows_match(R, F, K) == ts._rows_match(R, F, K)


@functools.lru_cache(maxsize=None)
def _placed_leg(G, K, R, F, track):
    """-> ((track, form) instances proven launched on G x K, problems).  One engine per gap form."""
    reads, refs, _, where = pm.batch(G, K, R, F)
    n = len(reads)
    d_reads, d_refs = torch.from_numpy(np.array(reads)).cuda(), torch.from_numpy(np.array(refs)).cuda()
    seen, problems = set(), []
    for form in pm.FORMS:
        args = pm.scoring_args(track, form, R, F, K)
        eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*args), group_lanes=G, rows_per_lane=K)
        try:
            assert eng.describe(0, n)["ran_placed_geometry"] == "none"
            got = eng.score_placed_device(0, d_reads, d_refs)
            torch.cuda.synchronize()
            got = got.cpu().numpy().astype(np.int64)
            d = eng.describe(0, n)
        finally:
            eng.close()
        instance = (track, pm.FORM_NAMES[form])
        what = (instance, args, d["ran_placed"], d["ran_placed_geometry"])
        exp = pm.reference(G, K, R, F, track, form)
        bad = np.nonzero((got != exp).any(axis=1))[0]
        if bad.size:
            problems.append(("records",) + what + (bad[:6].tolist(), got[bad[:4]].tolist(), exp[bad[:4]].tolist()))
        for p, (r, c) in where.items():            # the planted ties, from their construction
            if tuple(got[p]) != (args[0], r, c):
                problems.append(("planted tie",) + what + (p, got[p].tolist(), (args[0], r, c)))
        if instance in im.carried_placed(G, K):
            if d["ran_placed_geometry"] != "%dx%d" % (G, K) or d["ran_placed"] != track:
                problems.append(("not on its own geometry and track",) + what)
            else:
                seen.add(instance)
        else:
            # re-planned: correct, on a full geometry whose K answers the rule, and no coverage of this geometry
            g2 = _replanned_onto(d["ran_placed_geometry"], (G, K), R)
            if g2 is None:
                problems.append(("re-planned onto",) + what)
            elif d["ran_placed"] != tp._predict(R, F, args[0], g2[1], True):
                problems.append(("re-planned track",) + what + (tp._predict(R, F, args[0], g2[1], True),))
    return frozenset(seen), tuple(problems)


@pytest.mark.parametrize("leg", LEGS, ids=_leg_id)
def test_placed_instances(leg):
    seen, problems = _placed_leg(*leg)
    assert not problems, problems[:4]
    G, K, _, _, track = leg
    assert seen == {i for i in im.carried_placed(G, K) if i[0] == track}, sorted(seen)


@pytest.mark.parametrize("geom", GEOMS, ids=_geom_id)
def test_placed_coverage(geom):
    """The placed instances launched on the geometry are exactly the ones it carries, less instance_matrix.PLACED_UNSELECTABLE
    (empty: every one of the 68 can be selected at the matrix's shapes)."""
    seen, problems = set(), []
    for R, F in im.shapes(*geom):
        for track in pm.tracks(geom[1]):
            got, leg_problems = _placed_leg(geom[0], geom[1], R, F, track)
            seen |= got
            problems += leg_problems
    expected = im.carried_placed(*geom) - set(im.PLACED_UNSELECTABLE.get(geom, {}))
    assert seen == expected, ("never launched", sorted(expected - seen), "not expected", sorted(seen - expected), problems[:2])
    assert not problems, problems[:4]


def test_all_68_are_selectable():
    assert not im.PLACED_UNSELECTABLE and sum(len(im.carried_placed(*g)) for g in GEOMS) == 68


# ---- the re-plan at the key's edge: the forced geometry carries no kernel of the form, and the fallback's K has other bits ----
def _edge_matches(R, F, key_bits):
    """the last match inside and the first outside the key's range, for each number of key bits"""
    edges = []
    for bits in key_bits:
        inside = (32000 // (1 << bits) - 1) // min(R, F)
        assert ((min(R, F) * inside + 1) << bits) <= 32000 < ((min(R, F) * (inside + 1) + 1) << bits)
        edges += [inside, inside + 1]
    return edges


def _edge_pairs(R, F):
    """eight perfect hits (the largest value occurs) and sixteen related pairs as test_gpu_placed builds them"""
    reads, refs = synth.make_pairs(24, R, F, seed=R + F, sub_rate=0.0, n_run_frac=0.0, short_frac=0.0)
    reads[8:], refs[8:] = tp._pairs(16, R, F, 3)
    return reads, refs


@pytest.mark.parametrize("G,K,R,F,form,key_bits,matches", [(8, 4, 30, 100, "lin", (3, 2), (133, 134, 266, 267)),
                                                           (16, 12, 150, 200, "aff", (4, 3), (13, 14, 26, 27))])
def test_placed_replan_at_the_key_edge(G, K, R, F, form, key_bits, matches):
    """8 x 4 carries no kernel for gap_read != gap_ref and 16 x 12 none for four affine scores: every call re-plans, and the rule
    is asked again for the K it lands on.  At 30 rows, match 266 is the last inside 8 x 4's own two-bit key and outside the key of
    any geometry of more rows per lane, 133 the last inside a three-bit key; at 150 rows 13 is the last inside 16 x 12's own
    four-bit key and 26 the last inside a three-bit one.  The track that ran must be the rule's for the K that ran, whatever
    that K is -- and across the four matches both tracks must have been seen."""
    assert tuple(_edge_matches(R, F, key_bits)) == matches and im.placed_key_bits(K) in key_bits
    assert pm.FORM_NAMES[form] not in {f for _, f in im.carried_placed(G, K)}
    reads, refs = _edge_pairs(R, F)
    ran = set()
    for match in matches:
        sc = tp._scoring(form, match, -(match // 2))
        eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
        got = tp._run(eng, reads, refs)
        d = eng.describe(0, len(reads))
        eng.close()
        exp = placed_ref.placed(reads, refs, sc, affine=len(tp.FORMS[form]) > 2)
        assert exp[:8, 0].max() == min(R, F) * match            # perfect hits: the largest value the rule counts on occurs
        tp._check(got, exp, (G, K, form, match, d["ran_placed_geometry"]))
        g2 = _replanned_onto(d["ran_placed_geometry"], (G, K), R)
        assert g2 is not None, (match, d["ran_placed_geometry"])
        assert d["ran_placed"] == tp._predict(R, F, match, g2[1], True), (match, d["ran_placed"], d["ran_placed_geometry"])
        ran.add(d["ran_placed"])
    assert ran == {"key", "rows"}, ran


# ---- suboptimal and extension scores forced onto a geometry that carries none of their kernels ----
@pytest.mark.parametrize("geom", NOT_FULL, ids=_geom_id)
def test_subopt_replans_from_a_geometry_without_its_kernels(geom):
    G, K = geom
    assert not im.carried_subopt(G, K)
    R, F = G * K - K - 1, 2 * G + 7
    assert (R, F) in im.shapes(G, K)
    n = im.batch(G)
    reads, refs, _ = ts.cases.fuzz_batch(n, R, F, seed=R + F, plant_at=min(2, F - 1))
    reads = ts._trim_half(reads, np.random.default_rng(G * K))
    for form in ts.FORMS:
        sc = ts._scoring(form)
        prep = subopt_ref.prepare(reads, refs, sc, affine=ts._affine(form), chunk=64)
        eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
        assert eng.describe(0, n)["ran_subopt_geometry"] == "none"
        for mask in (0, G):
            ts._check(ts._run(eng, reads, refs, mask), subopt_ref.apply_mask(prep, mask), (G, K, R, F, form, mask))
        d = eng.describe(0, n)
        eng.close()
        g2 = _replanned_onto(d["ran_subopt_geometry"], geom, R)
        assert g2 is not None, (form, d["ran_subopt_geometry"])
        # (as test_gpu_subopt.test_every_instance expects them, for the geometry that ran)
        assert d["ran_subopt"] == tp._predict(R, F, 2, g2[1], True) and d["subopt_ring_cols"] == 4 * g2[0], (form, d["ran_subopt"], d["ran_subopt_geometry"], d["subopt_ring_cols"])
        assert d["ran_placed_geometry"] == "none" and d["ran_extend_geometry"] == "none"


@pytest.mark.parametrize("geom", NOT_FULL, ids=_geom_id)
def test_extend_replans_from_a_geometry_without_its_kernels(geom):
    G, K = geom
    assert not im.carried_extend(G, K)
    R, F = G * K - K - 1, 2 * G + 7
    n = im.batch(G)
    reads, refs = te._batch(n, R, F, seed=G * K + 5)
    for form in te.FORMS:
        sc = te._scoring(form)
        exp = extend_ref.extend(reads, refs, sc, affine=te._affine(form), chunk=16)
        eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
        assert eng.describe(0, n)["ran_extend_geometry"] == "none"
        got = te._run(eng, reads, refs)
        d = eng.describe(0, n)
        eng.close()
        te._check(got, exp, (G, K, R, F, form))
        assert d["ran_extend"] == "rows", (form, d["ran_extend"])
        assert _replanned_onto(d["ran_extend_geometry"], geom, R) is not None, (form, d["ran_extend_geometry"])
        assert d["ran_placed_geometry"] == "none" and d["ran_subopt_geometry"] == "none"
    assert (exp[:, 0] > 0).any() and (exp[:, 3] < 0).any()


def test_geometry_keys_off_the_register_sweep():
    """ "none" before any call, for the row strips, the int32 sweep and the banded chain, and after a refused call; a geometry
    after a register sweep"""
    R, F, n = 1025, 1300, 4
    reads, refs = tp._pairs(n, R, F, 8)
    eng = hipkernel.Engine(R, F, tp._scoring("sym"))
    d = eng.describe(0, n)
    assert (d["ran_placed_geometry"], d["ran_subopt_geometry"], d["ran_extend_geometry"]) == ("none", "none", "none")
    tp._run(eng, reads, refs)
    d = eng.describe(0, n)
    assert d["ran_placed"] == "strip" and d["ran_placed_geometry"] == "none", d
    eng.close()
    R, F, n = 64, 128, 8
    reads, refs = tp._pairs(n, R, F, 1)
    eng = hipkernel.Engine(R, F, tp._scoring("sym"))
    tp._run(eng, reads, refs)
    te._run(eng, reads, refs)
    ts._run(eng, reads, refs, 5)
    d = eng.describe(0, n)
    assert all(_geometry(d[k]) in im.GEOMETRIES for k in ("ran_placed_geometry", "ran_subopt_geometry", "ran_extend_geometry")), d
    narrow = tp._run(eng, reads, refs)
    eng.set_placed_wide(1)                  # the int32 sweep: not a register geometry's kernel
    eng.set_score_width(32)
    wide = tp._run(eng, reads, refs)
    d = eng.describe(0, n)
    assert d["ran_placed"] == "wide" and d["ran_placed_geometry"] == "none" and np.array_equal(wide, narrow), d
    eng.set_score_width(0)
    eng.set_placed_wide(0)
    tp._run(eng, reads, refs)
    assert _geometry(eng.describe(0, n)["ran_placed_geometry"]) in im.GEOMETRIES
    eng.set_traceback_policy(1)             # refused: each key falls back to "none" with its call
    for call in (lambda: tp._run(eng, reads, refs), lambda: te._run(eng, reads, refs), lambda: ts._run(eng, reads, refs, 5)):
        with pytest.raises(hipkernel.HipKernelError, match="traceback_policy"):
            call()
    d = eng.describe(0, n)
    assert (d["ran_placed_geometry"], d["ran_subopt_geometry"], d["ran_extend_geometry"]) == ("none", "none", "none"), d
    eng.close()
    R, F, n = 100, 120, 8                   # the banded block chain (a shape and band of tests/test_gpu_placed_band.py): no register geometry's kernel either
    reads, refs = tp._pairs(n, R, F, 2)
    eng = hipkernel.Engine(R, F, tp._scoring("sym"))
    tp._run(eng, reads, refs)
    assert _geometry(eng.describe(0, n)["ran_placed_geometry"]) in im.GEOMETRIES
    eng.set_band_width(8)
    eng.set_band_placed(1)
    tp._run(eng, reads, refs)
    d = eng.describe(0, n)
    assert d["ran_placed"] == "chain" and d["ran_placed_geometry"] == "none", d
    eng.close()
