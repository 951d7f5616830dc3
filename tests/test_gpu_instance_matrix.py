"""Every per-geometry score and fill kernel instance of libHIPKernel.so, launched through the public API on its own forced
geometry and compared bit for bit with the oracle (oracle/cpu_ref.c).

The cost model and cell_rules.h decide which instance a call launches; the rest of the suite reaches what they pick at its own
shapes.  Here each of the 17 geometries (tests/instance_matrix.py; tests/test_instance_matrix_table.py holds that table against
kernel_instances.hip.h) is forced, at shapes that exercise the geometry-dependent parts of a sweep -- padded lanes, overlapping
fill and drain, odd step counts, a partly filled second block -- and swept with a pool of scorings wide enough to select every
instance the geometry carries.  Which instance ran is read from describe() -- ran_score_geometry / ran_score_cells,
ran_align_geometry / ran_align_fill, set where the kernel pointer is taken -- and from plain facts of the scoring, never from a
copy of the selection rule.  Per geometry the instances seen must be exactly the ones it carries, less the two named in
instance_matrix.UNSELECTABLE."""
import functools
import re

import numpy as np
import pytest
import torch

import instance_matrix as im
from conftest import debug_switches
from oracle import cpu_ref
from versalignlib_amd import hipkernel, synth

pytestmark = pytest.mark.gpu

ALGS = ((hipkernel.SW, "SW"), (hipkernel.NW, "NW"))
GEOMS = sorted(im.GEOMETRIES)
CASES = [(G, K, R, F) for G, K in GEOMS for R, F in im.shapes(G, K)]
NO_TAG_CASES = [(G, K, R, F) for G, K in sorted(im.NEEDS_NO_TAG) for R, F in im.shapes(G, K)]


def _geom_id(g):
    return "%dx%d" % g


def _case_id(c):
    return "%dx%d-%dx%d" % c


def _is_affine(args):
    return len(args) > 4


def _is_symmetric(args):
    return args[4:6] == args[6:8] if _is_affine(args) else args[2] == args[3]


@functools.lru_cache(maxsize=None)
def _pairs(G, K, R, F):
    """Related pairs: mutated copies with indels, N runs, truncated (NUL-padded) pairs, lower case and junk bytes."""
    reads, refs = synth.make_pairs(im.batch(G), R, F, seed=7 * R + 131 * F + K, sub_rate=0.1, indel_rate=0.03, n_run_frac=0.15,
                                   short_frac=0.15, lowercase_frac=0.1, junk_frac=0.1)
    reads.setflags(write=False)
    refs.setflags(write=False)
    return reads, refs


@functools.lru_cache(maxsize=None)
def _ref_scores(G, K, R, F, args, alg):
    reads, refs = _pairs(G, K, R, F)
    exp = cpu_ref.score(alg, reads, refs, cpu_ref.Scoring.make(*args), threads=8, affine=_is_affine(args))
    exp.setflags(write=False)
    return exp


@functools.lru_cache(maxsize=None)
def _ref_alignments(G, K, R, F, args, alg, policy, wide):
    reads, refs = _pairs(G, K, R, F)
    rows, idx = cpu_ref.align(alg, reads, refs, cpu_ref.Scoring.make(*args), threads=8, affine=_is_affine(args),
                              policy="sse" if policy else "default", wide=wide)
    rows.setflags(write=False)
    idx.setflags(write=False)
    return rows, idx


def _score_form(alg_name, args, cells):
    """The gap form of the score_kernel instance that ran, from facts: the gap model, whether the two directions share
    their scores, and the cell format the launch reported."""
    if _is_affine(args):
        return ("AffineSym" if _is_symmetric(args) else "Affine") + ("F16" if cells == "f16" else "")
    if cells == "f16":
        # the NW half-float kernel has no gap constants left and serves unequal gaps too; SW has no such form
        assert alg_name == "NW" or _is_symmetric(args), ("SW, gap_read != gap_ref on half floats", args)
        return "SymF16"
    return "Sym" if _is_symmetric(args) else "Linear"


@functools.lru_cache(maxsize=None)
def _score_leg(G, K, R, F):
    """-> ((alg, form) instances proven launched on G x K, problems).  One engine per scoring of the pool; SW and NW, half
    floats on and off."""
    reads, refs = _pairs(G, K, R, F)
    n = reads.shape[0]
    d_reads, d_refs = torch.from_numpy(np.array(reads)).cuda(), torch.from_numpy(np.array(refs)).cuda()
    seen, problems = set(), []
    for args in im.SCORINGS:
        eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*args), group_lanes=G, rows_per_lane=K)
        try:
            assert eng.describe(0, n)["ran_score_geometry"] == "none"
            for alg, alg_name in ALGS:
                for half in (1, 0):
                    eng.set_half_float_cells(half)
                    # a scoring whose cells could leave int16 at this shape is swept on int32 cells by the strip kernels: not a
                    # register sweep, not this matrix's (tests/test_gpu_range_edges.py)
                    if eng.describe(alg, n)["score_cells"] == "int32":
                        continue
                    got = eng.score_device(alg, d_reads, d_refs).cpu().numpy()
                    d = eng.describe(alg, n)
                    what = (alg_name, args, "half" if half else "int", d["ran_score_geometry"], d["ran_score_cells"])
                    if d["ran_score_geometry"] != "%dx%d" % (G, K):
                        problems.append(("geometry",) + what)
                        continue
                    if d["ran_score_cells"] not in ("f16", "int16") or (not half and d["ran_score_cells"] != "int16"):
                        problems.append(("cells",) + what)
                        continue
                    exp = _ref_scores(G, K, R, F, args, alg)
                    bad = np.nonzero(got != exp)[0]
                    form = _score_form(alg_name, args, d["ran_score_cells"])
                    if bad.size:
                        problems.append(("scores", form) + what + (bad[:6].tolist(), got[bad[:6]].tolist(), exp[bad[:6]].tolist()))
                    seen.add((alg_name, form))
        finally:
            eng.close()
    return frozenset(seen), tuple(problems)


@functools.lru_cache(maxsize=None)
def _align_leg(G, K, R, F, no_tag):
    """-> ((alg, fill) instances proven launched on G x K, problems).  traceback_policy 0 for every scoring, 1 for the linear
    ones.  no_tag: the linear scorings again under the debug switch that takes the equality-test kernels."""
    reads, refs = _pairs(G, K, R, F)
    d_reads, d_refs = torch.from_numpy(np.array(reads)).cuda(), torch.from_numpy(np.array(refs)).cuda()
    seen, problems = set(), []
    with pytest.MonkeyPatch.context() as mp:
        if no_tag:
            debug_switches(mp, no_tag=1)
        for args in (im.LINEAR if no_tag else im.SCORINGS):
            eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*args), group_lanes=G, rows_per_lane=K)
            try:
                assert eng.describe(0, 1)["ran_align_geometry"] == "none"
                for policy in ((0,) if _is_affine(args) else (0, 1)):
                    eng.set_traceback_policy(policy)
                    for alg, alg_name in ALGS:
                        rows, idx = eng.align_device(alg, d_reads, d_refs)
                        rows, idx = rows.cpu().numpy(), idx.cpu().numpy()
                        d = eng.describe(alg, 1)
                        fill, geo = d["ran_align_fill"], d["ran_align_geometry"]
                        what = (alg_name, args, "policy", policy, fill, geo)
                        # (cells that could leave int16 take the int32 strips: the oracle's int32 cells then)
                        erows, eidx = _ref_alignments(G, K, R, F, args, alg, policy, fill.startswith("strip_wide"))
                        bad = np.nonzero((idx != eidx).any(axis=1) | (rows != erows).any(axis=(1, 2)))[0]
                        if bad.size:
                            problems.append(("alignments",) + what + (bad[:6].tolist(), idx[bad[:3]].tolist(), eidx[bad[:3]].tolist()))
                        if geo == "%dx%d" % (G, K):
                            seen.add((alg_name, fill))
                        elif geo == "none":
                            if not fill.startswith("strip"):
                                problems.append(("route",) + what)
                        else:
                            # re-planned onto a full geometry: correct, but no coverage of this one -- and only ever for a
                            # kernel this geometry does not carry
                            g2 = tuple(int(v) for v in geo.split("x"))
                            if not im.GEOMETRIES.get(g2, False) or (alg_name, fill) in im.carried_fills(G, K):
                                problems.append(("re-planned",) + what)
            finally:
                eng.close()
    return frozenset(seen), tuple(problems)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_score_instances(case):
    seen, problems = _score_leg(*case)
    assert not problems, problems[:4]
    assert seen, "no register sweep ran"


@pytest.mark.parametrize("geom", GEOMS, ids=_geom_id)
def test_score_coverage(geom):
    """All 14 score_kernel instances of the geometry were launched on it (and agreed with the oracle)."""
    seen, problems = set(), []
    for R, F in im.shapes(*geom):
        got, leg_problems = _score_leg(geom[0], geom[1], R, F)
        seen |= got
        problems += leg_problems
    assert seen == im.SCORE_INSTANCES, ("never launched", sorted(im.SCORE_INSTANCES - seen), "unknown", sorted(seen - im.SCORE_INSTANCES), problems[:2])
    assert not problems, problems[:4]


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_align_instances(case):
    seen, problems = _align_leg(*case, False)
    assert not problems, problems[:4]
    assert seen <= im.carried_fills(case[0], case[1]), sorted(seen - im.carried_fills(case[0], case[1]))


@pytest.mark.parametrize("case", NO_TAG_CASES, ids=_case_id)
def test_align_instances_no_tag(case):
    seen, problems = _align_leg(*case, True)
    assert not problems, problems[:4]
    assert seen and all(fill in ("linear", "linear_sym", "sse") for _, fill in seen), sorted(seen)


@pytest.mark.parametrize("geom", GEOMS, ids=_geom_id)
def test_align_coverage(geom):
    """The fill instances launched on the geometry are exactly the ones it carries, less instance_matrix.UNSELECTABLE: an
    instance nothing reaches fails here, and so does one of the two excluded ones should a call ever reach it."""
    seen, problems = set(), []
    for R, F in im.shapes(*geom):
        for no_tag in ((False, True) if geom in im.NEEDS_NO_TAG else (False,)):
            got, leg_problems = _align_leg(geom[0], geom[1], R, F, no_tag)
            seen |= got
            problems += leg_problems
    expected = im.carried_fills(*geom) - im.UNSELECTABLE.get(geom, frozenset())
    assert seen == expected, ("never launched", sorted(expected - seen), "not expected", sorted(seen - expected), problems[:2])
    assert not problems, problems[:4]


def test_geometry_keys_off_the_register_routes():
    """ "none" before any launch and for routes that are not a register sweep; a geometry otherwise."""
    R, F, n = 150, 200, 9
    reads, refs = synth.make_pairs(n, R, F, seed=3, indel_rate=0.02)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    eng = hipkernel.Engine(R, F)
    d = eng.describe(0, n)
    assert (d["ran_score_geometry"], d["ran_align_geometry"]) == ("none", "none")
    eng.score_device(0, d_reads, d_refs)
    eng.align_device(0, d_reads, d_refs)
    d = eng.describe(0, n)
    assert re.fullmatch(r"\d+x\d+", d["ran_score_geometry"]) and re.fullmatch(r"\d+x\d+", d["ran_align_geometry"]), d
    assert tuple(int(v) for v in d["ran_score_geometry"].split("x")) in im.GEOMETRIES
    eng.set_score_width(32)                 # int32 cells: the strip kernels
    got = eng.score_device(0, d_reads, d_refs).cpu().numpy()
    d = eng.describe(0, n)
    assert d["ran_score_cells"] == "int32" and d["ran_score_geometry"] == "none", d
    assert np.array_equal(got, cpu_ref.score(0, reads, refs, threads=4))
    eng.close()
    # a scoring whose alignment cells leave int16: int32 strips, no register fill
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(400, -300, -350, -350))
    eng.align_device(0, d_reads, d_refs)
    d = eng.describe(0, n)
    assert d["ran_align_fill"] == "strip_wide" and d["ran_align_geometry"] == "none", d
    eng.close()
