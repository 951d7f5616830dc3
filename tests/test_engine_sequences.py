"""The generator of tests/engine_sequences.py on the CPU: the committed (world, seed) sequences are deterministic and hold what
tests/test_gpu_engine_sequences.py relies on.  These are conditions on the generator, not measurements: a seed that misses one
fails here, before any GPU run.

Three more things that need no GPU.  extension_route() -- the model's restatement of the rule that sends the two extension
families to the BANDED int32 strip sweep -- is held to its truth table, and the predicates that recognise the orders sharing
state to hand-made lists.  The pools are held to what the Band route needs of its inputs (test_the_pools_exercise_the_band): a
band that changes records, read ends both reached and unreached, and in the strips world best cells in the second 512-row strip;
these take the banded references of every (world, scoring, band) -- seconds each at 520 x 600, the one deliberate exception to
quick tests here, since no smaller shape has two strips.  And the runner's verify() is held to two mutants
(test_verify_tells_the_band_route_from_its_neighbours): it runs without torch through Runner(..., device=False)."""
import functools

import numpy as np
import pytest

import engine_sequences as es

CASES = [(world, seed) for world in sorted(es.WORLDS) for seed in es.WORLDS[world]["seeds"]]


@pytest.mark.parametrize("world,seed", CASES)
def test_the_sequence_is_a_pure_function(world, seed):
    a, b = es.sequence(world, seed), es.sequence(world, seed)
    assert a == b and a is not b
    assert es.sequence(world, seed + 1000) != a
    for step in a:
        if step["kind"] == "set":
            assert step["key"] in es.KEYS and step["value"] in es.key_values(world, step["key"])
        else:
            assert step["kind"] == "call" and step["entry"] in es.ENTRY_POINTS and step["alg"] in (es.SW, es.NW)
            assert step["n"] in es.LADDER and 0 <= step["begin"] and step["begin"] + step["n"] <= es.POOL
            assert 1 <= step["threads"] <= 3 and step["mask"] >= 0 and step["extended"] in (0, 1)
            assert step["end_bonus"] in es.END_BONUSES and step["with_extend"] in (0, 1)


@pytest.mark.parametrize("world,seed", CASES)
def test_every_sequence_moves_every_key_and_makes_every_call(world, seed):
    steps = es.sequence(world, seed)
    calls = [s for s in steps if s["kind"] == "call"]
    assert len(steps) >= 60 and len(calls) >= 40, (len(steps), len(calls))
    # every setter changes value at least once and returns to an earlier value at least once
    state = es.initial_state()
    history = {k: [v] for k, v in state.items()}
    for s in steps:
        if s["kind"] == "set":
            assert s["value"] != state[s["key"]], ("a key change that changes nothing", s)
            state = es.apply_step(state, s)
            history[s["key"]].append(s["value"])
    for key in es.KEYS:
        h = history[key]
        assert len(h) >= 2, (key, "never changes")
        assert any(h[i] in h[:i] for i in range(1, len(h))), (key, "never returns to an earlier value", h)
    # ... and the model says what the library does with pointer_scratch_cap_mb = 0: nothing, so the state never goes back there
    assert 0 not in history["pointer_scratch_cap_mb"][1:]
    with pytest.raises(ValueError):
        es.apply_step(state, {"kind": "set", "key": "pointer_scratch_cap_mb", "value": 0})
    for entry in es.ENTRY_POINTS:
        assert sum(1 for c in calls if c["entry"] == entry) >= 3, entry
    # at least one call follows a band_width step that went from a positive width to 0
    band, cleared, used = 0, False, False
    for s in steps:
        if s["kind"] == "set" and s["key"] == "band_width":
            cleared = cleared or (band > 0 and s["value"] == 0)
            band = s["value"]
        elif s["kind"] == "call" and cleared:
            used = True
    assert used
    assert {s["n"] for s in calls} == set(es.LADDER)
    # the fields only the new CIGAR families read take every value there
    extend_align = [c for c in calls if es.FAMILY_OF[c["entry"]] == "extend_align"]
    assert {c["end_bonus"] for c in extend_align} == set(es.END_BONUSES) == {-1, 0, 5, 2 ** 31 - 1}
    assert {c["with_extend"] for c in extend_align} == {0, 1}
    assert {c["extended"] for c in calls if es.FAMILY_OF[c["entry"]] == "span_cigar"} == {0, 1}


def test_the_model_holds_the_whole_library():
    """the key, the eighteen entry points and the nine families"""
    from versalignlib_amd import hipkernel
    assert len(es.KEYS) == 15 and len(set(es.KEYS)) == 15 and set(es.KEYS) == set(es.DEFAULTS) and set(es.ECHOED) <= set(es.KEYS)
    for key in ("extend_wide", "extend_band", "extend_band_align"):
        assert es.DEFAULTS[key] == 0 and key in es.ECHOED and es.key_values("short", key) == (0, 1), key
    assert "extend_band_block_rows" in es.PLAN_KEYS
    assert len(es.FAMILIES) == 9 and len(es.ENTRY_POINTS) == 18 and len(set(es.ENTRY_POINTS)) == 18
    assert es.ENTRIES_OF["span_cigar"] == ("align_span_device", "align_span_host")
    assert es.ENTRIES_OF["extend"] == ("score_extend_device", "score_extend_host")
    assert es.ENTRIES_OF["extend_align"] == ("align_extend_device", "align_extend_host")
    for key in es.KEYS:
        assert callable(getattr(hipkernel.Engine, "set_" + key)), key
    for entry in es.ENTRY_POINTS:
        assert callable(getattr(hipkernel.Engine, entry)), entry
    assert set(es.RAN_KEYS) == set(es.FAMILIES)
    for (world, scoring), entries in es.NEVER_SUCCEEDS.items():
        assert scoring in es.WORLDS[world]["scorings"] and set(entries) <= set(es.ENTRY_POINTS)
        assert tuple(entries) == es.ENTRIES_OF["subopt"] == ("score_subopt_device", "score_subopt_host")
    assert set(es.NEVER_SUCCEEDS) == {("long", s) for s in es.WORLDS["long"]["scorings"]} | {("short", "wide")}
    for world in es.WORLDS:             # the Band route runs extension alignments in every world: only the suboptimal scores stay capped
        assert es.capped_families(world) == {"subopt"}, world
    assert es.CALLS >= 60


SEEDED = sorted(world for world in es.WORLDS if es.WORLDS[world]["seeds"])
EXTENSIONS = ("extend", "extend_align")


def test_the_extension_route_restates_the_header():
    """include/valign_hip.h: the scores answer band iff band_width > 0 and extend_band == 1, the alignments iff in addition
    extend_band_align == 1; with band_width == 0 neither key is read"""
    for band in (0, 16):
        for eb in (0, 1):
            for eba in (0, 1):
                state = dict(es.initial_state(), band_width=band, extend_band=eb, extend_band_align=eba)
                scores, aligns = es.extension_route(state, "extend"), es.extension_route(state, "extend_align")
                if band == 0:
                    assert scores == aligns == "unbanded"
                else:
                    assert scores == ("band" if eb else "refused") and aligns == ("band" if eb and eba else "refused")
                # no other key moves the route
                for key in es.KEYS:
                    if key not in ("band_width", "extend_band", "extend_band_align"):
                        for value in es.key_values("short", key):
                            assert es.extension_route(dict(state, **{key: value}), "extend_align") == aligns
    with pytest.raises(ValueError):
        es.extension_route(es.initial_state(), "placed")
    # what the Band route itself refuses is not "runs banded"
    on = dict(es.initial_state(), band_width=16, extend_band=1, extend_band_align=1)
    call = {"alg": es.SW}
    assert es.runs_banded("extend_align", on, call) and es.runs_banded("extend", dict(on, extend_band_align=0, score_width=32), call)
    assert not es.runs_banded("extend", dict(on, score_width=16), call) and not es.runs_banded("extend", dict(on, traceback_policy=1), call)
    assert not es.runs_banded("extend", on, {"alg": es.NW}) and not es.runs_banded("extend_align", dict(on, extend_band_align=0), call)
    assert not es.runs_banded("placed", on, call)


@pytest.mark.parametrize("world", SEEDED)
def test_the_band_route_shares_state_in_every_order(world):
    """Per world, over its seeds: the four orders in which the Band route of the extension families meets the state it shares --
    the strip scratch under three layouts (all six ordered pairs), the pointer and rows scratch around unbanded CIGARs, two bands
    on one engine, a band cleared and set again between extension calls -- and every end_bonus and with_extend ON that route."""
    pairs, pointer, two, cleared, bonuses, with_extend = set(), False, False, False, set(), set()
    for seed in es.WORLDS[world]["seeds"]:
        made = es.calls_with_state(es.sequence(world, seed))
        pairs |= es.strip_scratch_neighbours(made)
        pointer = pointer or es.pointer_scratch_order(made)
        two = two or es.two_bands_order(made)
        cleared = cleared or es.band_cleared_order(made)
        for family, state, step in made:
            if family == "extend_align" and es.runs_banded(family, state, step):
                bonuses.add(step["end_bonus"])
                with_extend.add(step["with_extend"])
    assert pairs == es.STRIP_SCRATCH_ORDERS and len(es.STRIP_SCRATCH_ORDERS) == 6, sorted(es.STRIP_SCRATCH_ORDERS - pairs)
    assert pointer, "no banded extension alignment between two unbanded CIGAR calls"
    assert two, "no banded extension alignments under one band, the other, the first again"
    assert cleared, "no banded extension call before and after an extension call under band_width = 0"
    assert bonuses == set(es.END_BONUSES) and with_extend == {0, 1}, (bonuses, with_extend)


def test_the_order_predicates_tell_orders_apart():
    """the predicates above on hand-made lists of calls: each is true on its order and false on the nearest miss"""
    on = dict(es.initial_state(), band_width=16, extend_band=1, extend_band_align=1)
    other = dict(on, band_width=40)
    wide = dict(es.initial_state(), placed_wide=1, score_width=32)
    sw = {"alg": es.SW}
    A, E, P, C = ("extend_align", on, sw), ("extend", on, sw), ("placed", wide, sw), ("cigar", es.initial_state(), sw)
    assert es.strip_scratch_neighbours([P, E, A, P, A, E, P]) == es.STRIP_SCRATCH_ORDERS
    assert es.strip_scratch_neighbours([P, E, A, P]) == {("placed", "extend"), ("extend", "extend_align"), ("extend_align", "placed")}
    assert es.strip_scratch_neighbours([("placed", dict(wide, score_width=0), sw), E]) == set()         # (not the int32 sweep by the keys alone)
    assert es.strip_scratch_neighbours([("placed", dict(wide, band_width=16), sw), E]) == set()
    assert es.strip_scratch_neighbours([P, ("extend", dict(on, extend_band=0), sw)]) == set()
    assert es.pointer_scratch_order([C, A, C]) and es.pointer_scratch_order([("cigar", dict(on, band_alignments=0), sw), A, C])
    assert not es.pointer_scratch_order([C, A, ("cigar", dict(on, band_alignments=1), sw)]) and not es.pointer_scratch_order([C, E, C])
    assert not es.pointer_scratch_order([C, ("extend_align", es.initial_state(), sw), C])
    B = ("extend_align", other, sw)
    assert es.two_bands_order([A, B, A]) and not es.two_bands_order([A, A, A]) and not es.two_bands_order([A, B, B]) and not es.two_bands_order([A, C, B, A])
    plain = ("extend", es.initial_state(), sw)
    assert es.band_cleared_order([E, plain, A]) and not es.band_cleared_order([E, A, plain]) and not es.band_cleared_order([E, C, A])


@pytest.mark.parametrize("world,seed", CASES)
def test_every_sequence_calls_the_band_route_and_its_refusals(world, seed):
    """Per sequence: at least three calls of each extension family in a state whose route is "band", every extension entry point
    at least twice where the model expects the Band route to RUN (what the GPU test asserts of the runner's per-route counts), and
    at least one call of each family under a band with the keys off."""
    made = es.calls_with_state(es.sequence(world, seed))
    for family in EXTENSIONS:
        mine = [(state, step) for f, state, step in made if f == family]
        assert sum(1 for state, _ in mine if es.extension_route(state, family) == "band") >= 3, family
        assert sum(1 for state, _ in mine if es.extension_route(state, family) == "refused") >= 1, family
        for entry in es.ENTRIES_OF[family]:
            assert sum(1 for state, step in mine if step["entry"] == entry and es.runs_banded(family, state, step)) >= 2, entry
            # ... and the routes without a band keep their share, wherever one of them can serve the entry point: not the long
            # world's alignments, which only the Band route runs
            unbanded = sum(1 for state, step in mine if step["entry"] == entry and step["alg"] == es.SW and _unbanded_route_serves(world, family, state))
            assert unbanded >= 2 or (world == "long" and family == "extend_align"), (entry, unbanded)


def _unbanded_route_serves(world, family, state):
    """include/valign_hip.h, for some scoring of the world: without a band and under traceback_policy = 0 the register route serves
    an extension alignment unless score_width = 32 asks for int32 cells; an extension score runs on the register route of the tiny
    world under the same condition, and everywhere under extend_wide = 1 -- but for score_width = 16 ("int16 or refuse") where
    the shape is not one of the long reads that the key moves whatever score_width says."""
    if state["band_width"] or state["traceback_policy"]:
        return False
    if family == "extend_align":
        return world != "long" and state["score_width"] != 32
    return (world == "tiny" and state["score_width"] != 32) or (state["extend_wide"] == 1 and (state["score_width"] != 16 or world == "long"))


@pytest.mark.parametrize("world", SEEDED)
def test_the_orders_that_share_state_occur(world):
    """Per world, over its seeds: the orders in which two families use one piece of the engine -- the spanned calls' child
    engine, the CIGAR rows scratch at its two pitches, the strip scratch of the two int32 sweeps -- with batch sizes from the
    ladder on both sides."""
    triples, wide = set(), False
    for seed in es.WORLDS[world]["seeds"]:
        made = es.calls_with_state(es.sequence(world, seed))
        assert all(step["n"] in es.LADDER for _, _, step in made)
        families = [f for f, _, _ in made]
        triples |= set(zip(families, families[1:], families[2:]))
        for (fa, sa, _), (fb, sb, _) in zip(made, made[1:]):
            if {fa, fb} == {"placed", "extend"}:
                placed, extend = (sa, sb) if fa == "placed" else (sb, sa)
                wide = wide or (placed["placed_wide"] == 1 and extend["extend_wide"] == 1)
    assert ("span", "span_cigar", "span") in triples
    assert ("cigar", "extend_align", "cigar") in triples
    assert wide, "no placed call under placed_wide = 1 next to an extension-score call under extend_wide = 1"


@pytest.mark.parametrize("world", SEEDED)
def test_every_ordered_pair_of_families_is_neighbours_somewhere(world):
    seen = set()
    for seed in es.WORLDS[world]["seeds"]:
        calls = [s for s in es.sequence(world, seed) if s["kind"] == "call"]
        seen |= {(es.FAMILY_OF[a["entry"]], es.FAMILY_OF[b["entry"]]) for a, b in zip(calls, calls[1:])}
    missing = [(a, b) for a in es.FAMILIES for b in es.FAMILIES if a != b and (a, b) not in seen]
    assert not missing, missing


def test_the_worlds_are_what_the_gpu_test_says():
    assert set(es.WORLDS) == {"short", "long", "tiny", "strips"}
    strips = es.WORLDS["strips"]
    # no generated sequences; a read longer than one 512-row strip, and a reference that outlasts it: the read end lies in the band
    assert strips["seeds"] == () and strips["R"] == 520 > 512 and strips["F"] == 600 > strips["R"] and strips["bands"] == (40, 130)
    assert strips["scorings"] == ("linear", "sym_affine", "affine4")
    assert len({es._STREAM_OF[world] for world in es.WORLDS}) == 4
    for world, w in es.WORLDS.items():
        assert len(w["seeds"]) == (0 if world == "strips" else 3) and {"linear", "sym_affine", "affine4"} <= set(w["scorings"])
        assert len(w["bands"]) == 2 and 0 < w["bands"][0] < w["bands"][1]
        assert ("wide" in w["scorings"]) == (world == "short")
        assert es.pairs(world)[0].shape == (es.POOL, w["R"]) and es.pairs(world)[1].shape == (es.POOL, w["F"])
        assert max(es.LADDER) <= 130 and max(es.LADDER) <= es.POOL
    assert es.WORLDS["long"]["R"] > 3 * 512 and es.WORLDS["tiny"]["R"] < 16
    a4 = es.SCORINGS["affine4"]
    assert len(set(a4[4:])) == 4 and a4[5] >= a4[4] and a4[7] >= a4[6]
    assert es.SCORINGS["sym_affine"][4:6] == es.SCORINGS["sym_affine"][6:8]
    assert es.SCORINGS["wide"][0] == 600


# ---- the inputs of the Band route, from the references alone: without these a passing GPU run proves nothing ----
@functools.lru_cache(maxsize=None)
def _comparer(world, scoring):
    return es.Runner(world, scoring, device=False)          # the references and verify(): no torch, no GPU


UNREACHED = -(1 << 31)          # VALIGN_HIP_EXTEND_UNREACHED


@pytest.mark.parametrize("world,scoring", [(world, scoring) for world in sorted(es.WORLDS) for scoring in es.WORLDS[world]["scorings"]],
                         ids=lambda v: str(v))
def test_the_pools_exercise_the_band(world, scoring):
    """For every band of the world: the banded score reference differs from the unbanded one on at least 8 pairs of the pool (a
    call that quietly ran unbanded fails), some read end is unreached, and -- outside the long world, whose band ends near row 130
    of 1600 -- at least 100 are reached; the long world holds at least 150 unreached ones.  strips: at least 60 best cells below
    row 512 (the second strip's rows carry the result) and alignment records that depend on the end-bonus rule on at least 30
    pairs.  Measured with today's pools -- tiny: unreached 3 / 1, differs 54-81 / 8-31; short: unreached 7 / 6, differs >= 84;
    long: unreached 159 / 158; strips: unreached 18 / 16, differs 116-121 / 36-38, best row > 512 on 74-114 pairs, records
    differing on 89-96 / 32-39 pairs."""
    r = _comparer(world, scoring)
    free = r.ref_extend()
    assert free.shape == (es.POOL, 5)
    for band in es.WORLDS[world]["bands"]:
        banded = r.ref_extend_band(band)
        differs = int((banded != free).any(axis=1).sum())
        unreached = int((banded[:, 3] == UNREACHED).sum())
        print(world, scoring, "band", band, "differs", differs, "unreached", unreached)
        assert differs >= 8, (band, differs)
        assert unreached >= 1, band
        if world == "long":
            assert unreached >= 150, (band, unreached)
        else:
            assert es.POOL - unreached >= 100, (band, unreached)
        if world == "strips":
            below = int((banded[:, 1] > 512).sum())
            by_bonus = r.ref_extend_band_align(band, 1)
            depends = int((by_bonus[-1][0] != by_bonus[2 ** 31 - 1][0]).any(axis=1).sum())
            print(world, scoring, "band", band, "best cells below row 512", below, "records that depend on the end bonus", depends)
            assert below >= 60, (band, below)
            assert depends >= 30, (band, depends)
            # the extension records of the alignment reference are the score reference's: one definition, restated twice
            assert np.array_equal(by_bonus[5][2], banded)


# ---- the runner itself: verify() must tell the Band route's results from their nearest neighbours ----
def _device_layout(r, recs, ops, ext):
    """a reference result in the layout align_extend_device returns: int32 records, sentinel-filled op rows, extension records"""
    got_ops = np.full((len(recs), r.stride), es.SENTINEL, np.int32)
    for p, pair_ops in enumerate(ops):
        got_ops[p, :len(pair_ops)] = np.array(pair_ops, np.uint32).view(np.int32)
    return recs.astype(np.int32), got_ops, ext.astype(np.int32)


def test_verify_tells_the_band_route_from_its_neighbours():
    """Two mutants, on a 130-pair slice of the short world: the UNBANDED extension records handed in where the banded reference
    is expected, and a banded alignment result whose extension records say gscore = 0 where the read end is UNREACHED.  verify()
    raises SequenceMismatch for both, and accepts the unmutated results."""
    r = _comparer("short", "linear")
    band, b, n = es.WORLDS["short"]["bands"][0], 3, 130
    free, banded = r.ref_extend()[b:b + n], r.ref_extend_band(band)[b:b + n]
    step = {"entry": "score_extend_device", "begin": b, "n": n}
    r.verify(step, (banded.astype(np.int32),), (banded,), "control")
    with pytest.raises(es.SequenceMismatch, match="differs from the reference"):
        r.verify(step, (free.astype(np.int32),), (banded,), "unbanded for banded")
    recs, ops, _, _, _ = r.ref_extend_band_align(band, 1)[5]
    exp = (recs[b:b + n], ops[b:b + n], banded)
    step = {"entry": "align_extend_device", "begin": b, "n": n}
    r.verify(step, _device_layout(r, *exp), exp, "control")
    hit = banded[:, 3] == UNREACHED
    assert hit.any(), "no unreached read end in the slice"
    mutant = banded.copy()
    mutant[hit, 3] = 0
    with pytest.raises(es.SequenceMismatch, match="extension records differ"):
        r.verify(step, _device_layout(r, exp[0], exp[1], mutant), exp, "gscore 0 for UNREACHED")
    # ... and the host layout: structured records, packed ops, offsets
    offsets = np.concatenate([[0], np.cumsum([len(o) for o in exp[1]])]).astype(np.int64)
    flat = np.array([o for pair_ops in exp[1] for o in pair_ops], np.uint32)

    def structured(values, dtype):
        out = np.zeros(len(values), dtype)
        for k, name in enumerate(dtype.names):
            out[name] = values[:, k]
        return out
    step = {"entry": "align_extend_host", "begin": b, "n": n}
    host = (structured(exp[0], r.hk.aln_dtype()), flat, offsets)
    r.verify(step, host + (structured(banded, r.hk.extend_dtype()),), exp, "control")
    with pytest.raises(es.SequenceMismatch, match="extension records differ"):
        r.verify(step, host + (structured(mutant, r.hk.extend_dtype()),), exp, "gscore 0 for UNREACHED, host")
