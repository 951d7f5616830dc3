"""The generator of tests/engine_sequences.py on the CPU: the committed (world, seed) sequences are deterministic and hold what
tests/test_gpu_engine_sequences.py relies on.  These are conditions on the generator, not measurements: a seed that misses one
fails here, before any GPU run."""
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
    assert len(es.KEYS) == 13 and set(es.KEYS) == set(es.DEFAULTS) and es.DEFAULTS["extend_wide"] == 0 and set(es.ECHOED) <= set(es.KEYS)
    assert "extend_wide" in es.ECHOED and es.key_values("short", "extend_wide") == (0, 1)
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
        assert set(entries) == set(es.ENTRIES_OF["subopt"] + es.ENTRIES_OF["extend_align"])
    assert set(es.NEVER_SUCCEEDS) == {("long", s) for s in es.WORLDS["long"]["scorings"]} | {("short", "wide")}
    assert es.capped_families("tiny") == {"subopt"} and es.capped_families("long") == es.capped_families("short") == {"subopt", "extend_align"}
    assert es.CALLS >= 60


@pytest.mark.parametrize("world", sorted(es.WORLDS))
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


@pytest.mark.parametrize("world", sorted(es.WORLDS))
def test_every_ordered_pair_of_families_is_neighbours_somewhere(world):
    seen = set()
    for seed in es.WORLDS[world]["seeds"]:
        calls = [s for s in es.sequence(world, seed) if s["kind"] == "call"]
        seen |= {(es.FAMILY_OF[a["entry"]], es.FAMILY_OF[b["entry"]]) for a, b in zip(calls, calls[1:])}
    missing = [(a, b) for a in es.FAMILIES for b in es.FAMILIES if a != b and (a, b) not in seen]
    assert not missing, missing


def test_the_worlds_are_what_the_gpu_test_says():
    assert set(es.WORLDS) == {"short", "long", "tiny"}
    for world, w in es.WORLDS.items():
        assert len(w["seeds"]) == 3 and {"linear", "sym_affine", "affine4"} <= set(w["scorings"])
        assert ("wide" in w["scorings"]) == (world == "short")
        assert es.pairs(world)[0].shape == (es.POOL, w["R"]) and es.pairs(world)[1].shape == (es.POOL, w["F"])
        assert max(es.LADDER) <= 130 and max(es.LADDER) <= es.POOL
    assert es.WORLDS["long"]["R"] > 3 * 512 and es.WORLDS["tiny"]["R"] < 16
    a4 = es.SCORINGS["affine4"]
    assert len(set(a4[4:])) == 4 and a4[5] >= a4[4] and a4[7] >= a4[6]
    assert es.SCORINGS["sym_affine"][4:6] == es.SCORINGS["sym_affine"][6:8]
    assert es.SCORINGS["wide"][0] == 600
