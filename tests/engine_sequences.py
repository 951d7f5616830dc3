"""Sequences of key changes and calls for ONE long-lived hipkernel.Engine, and the runner that holds such an engine against the
references and against new engines (tests/test_engine_sequences.py, tests/test_gpu_engine_sequences.py,
tools/fuzz_device.py --kind sequence).

Every other GPU test creates an engine, sets its keys once, makes one kind of call and closes it.  A host keeps one engine for
hours and flips band_width, score_width and traceback_policy between calls, and the engine carries plans, tables, contexts,
pipeline state and grow-only scratch from call to call (class Engine, versalignlib_amd/csrc/engine.hip.h).  Here:

  sequence(world, seed) ... a pure function -> a list of steps, drawn from synth._stream.  A step is a key change (one setter,
                            one new value) or a call (entry point, algorithm, a slice of the world's pairs, threads / mask /
                            extended / end_bonus / with_extend where the entry point reads them).
  State ................... the current value of every key; configure(engine, state) applies one to a new engine.
  Runner .................. one engine runs the whole sequence on one non-default stream; every call is held, bit for bit,
                            against the reference of the operation the state selects, and against a NEW engine configured to
                            the same state that makes the same call on the same data.

Nine families of entry points share the engine: scores, alignment rows, CIGARs, placed, spanned and suboptimal scores, spanned
CIGARs, extension scores and extension alignments.  The last three came with the most shared scratch: spanned scores and
spanned CIGARs re-key ONE child engine, each with its own set of keys; extension alignments walk in the rows scratch of the
CIGAR calls at another row pitch; extension scores under extend_wide sweep on the boundary rows of the placed int32 sweep.

The two newest keys, extend_band and extend_band_align, move the two extension families to the BANDED int32 strip sweep under
band_width > 0 (extension_route() restates the rule of include/valign_hip.h).  That route lies on more shared, grow-only state
than any before it: its boundary rows and partial records are the strip scratch of the placed int32 sweep, of extend_wide and of
the placed strip route -- three record layouts --, its pointer regions and end cells the pointer scratch of every alignment fill,
its walk the CIGAR rows scratch at a pitch of R + F + 1.  The references there are tests/extend_band_ref.py and
tests/extend_band_align_ref.py, and expected() asserts that the route describe() reports is the one the rule names before it
picks a reference.  A fourth world, strips (520 x 600), exists for the hand-written sequences only: the smallest shape at which a
read crosses a 512-row strip boundary and still reaches its end inside the band.

describe() is host-side state -- with one exception: after a score call whose last launch ran on the 8 x 19 side tile it reports
"ran_score_sym_affine_form" from two words the kernels wrote, and waits for the DEVICE to read them (Engine::ran_side_tile_form).
The short world's 150-row reads under sym_affine are that tile's window: a length-sorted score call with half_float_cells = 0
takes it there, and from then until the next score call that runs elsewhere every describe() drains the stream.  Runner.run
therefore reads describe() late, behind the wait it makes anyway, wherever the very next step settles.

The generator needs no GPU; the runner imports torch when it is created."""
import functools

import numpy as np

from versalignlib_amd import synth

SW, NW = 0, 1

# ---- the model of the state -------------------------------------------------------------------------------------------------
KEYS = ("band_width", "band_alignments", "band_nw", "band_placed", "placed_wide", "extend_wide", "extend_band", "extend_band_align",
        "trace_checkpoints", "score_width", "traceback_policy", "ragged_batching", "host_packing", "half_float_cells", "pointer_scratch_cap_mb")
DEFAULTS = {"band_width": 0, "band_alignments": 0, "band_nw": 0, "band_placed": 0, "placed_wide": 0, "extend_wide": 0, "extend_band": 0,
            "extend_band_align": 0, "trace_checkpoints": 0, "score_width": 0, "traceback_policy": 0, "ragged_batching": 0, "host_packing": 1,
            "half_float_cells": 1, "pointer_scratch_cap_mb": 0}
# pointer_scratch_cap_mb can only be SET: 0 means "leave the cap as it is" to the library, so the state never returns to 0
SET_ONLY_POSITIVE = ("pointer_scratch_cap_mb",)

FAMILIES = ("score", "rows", "cigar", "placed", "span", "subopt", "span_cigar", "extend", "extend_align")
ENTRIES_OF = {"score": ("score_device", "score_host"), "rows": ("align_device", "align_host"),
              "cigar": ("align_cigar_device", "align_cigar_host"), "placed": ("score_placed_device", "score_placed_host"),
              "span": ("score_span_device", "score_span_host"), "subopt": ("score_subopt_device", "score_subopt_host"),
              "span_cigar": ("align_span_device", "align_span_host"), "extend": ("score_extend_device", "score_extend_host"),
              "extend_align": ("align_extend_device", "align_extend_host")}
ENTRY_POINTS = tuple(e for f in FAMILIES for e in ENTRIES_OF[f])
FAMILY_OF = {e: f for f in FAMILIES for e in ENTRIES_OF[f]}

LADDER = (1, 7, 40, 130)            # batch sizes: scratch buffers are reused, regrown and reused smaller
POOL = 160                          # pairs of a world; a call takes a slice of them
CALLS = 64                          # calls drawn per sequence (the repairs at the end add some forty): with fifteen keys the tiny
                                    # world's seeds still missed one of the 72 ordered pairs of families as neighbours at 62
SUBOPT_CALLS = 6                    # ... of which suboptimal ones, and of every family capped_families() names: each of their calls is refused
                                    # by definition under some scoring of the world, and would eat the budget of refusals
END_BONUSES = (-1, 0, 5, 2 ** 31 - 1)       # extension alignments: the best cell, the rule in between (twice), always the read end

# The smallest shapes at which each route still exists.  short: the register sweep, the fused / direct small host calls, the
# ragged classes, the block chain under a band.  long: plan_ is the long plan by construction, alignments take the row strips
# on four 512-row strips, placed scores the strip route.  tiny: fewer rows than any geometry has.
# Under the band of the extension families (the anchor's diagonal i = j) the long world's band ends near row 130 of its 1600: 159 /
# 158 of its 160 pairs have an UNREACHED read end at bands 24 / 64.  It covers the unreached rule, the four strips with empty
# windows behind the first and the sizes of the strip scratch -- and nothing else of the banded walk.  strips is the smallest shape
# at which a read crosses a 512-row strip boundary AND reaches its end inside the band (F > R: the reference outlasts the read): 142 /
# 144 reached read ends, 74 and more best cells below row 512.  It has no seeds -- no generated sequences -- and is used by the
# hand-written sequences only: its references take seconds on the CPU for the whole pool, and are computed lazily like all others.
WORLDS = {
    "short": {"R": 150, "F": 200, "bands": (16, 40), "scorings": ("linear", "sym_affine", "affine4", "wide"), "seeds": (1, 2, 3)},
    "long": {"R": 1600, "F": 96, "bands": (24, 64), "scorings": ("linear", "sym_affine", "affine4"), "seeds": (1, 2, 3)},
    "tiny": {"R": 12, "F": 20, "bands": (4, 12), "scorings": ("linear", "sym_affine", "affine4"), "seeds": (1, 2, 3)},
    "strips": {"R": 520, "F": 600, "bands": (40, 130), "scorings": ("linear", "sym_affine", "affine4"), "seeds": ()},
}
_STREAM_OF = {"long": 1, "short": 2, "tiny": 3, "strips": 4}       # the generator's stream per world: a new world moves no other's
# match, mismatch, gap_read, gap_ref [, open_read, ext_read, open_ref, ext_ref]; wide: cells leave int16 at 150 x 200
SCORINGS = {"linear": (2, -1, -3, -3), "sym_affine": (2, -1, -3, -3, -5, -1, -5, -1), "affine4": (2, -1, -3, -3, -6, -1, -4, -2),
            "wide": (600, -1, -3, -3)}
# Entry points that no state lets succeed (include/valign_hip.h, "REFUSED" of the suboptimal scores): reads of more than
# 1 024 rows take the row strips, and a shape x scoring whose cells can leave int16 is refused whatever placed_wide says
NEVER_SUCCEEDS = {("long", s): ENTRIES_OF["subopt"] for s in WORLDS["long"]["scorings"]}
NEVER_SUCCEEDS[("short", "wide")] = ENTRIES_OF["subopt"]
# (Nothing else.  Extension scores run under extend_wide = 1 wherever the register sweep refuses them here -- 96 x 2 and 150 x
# 600 are far below 2^28.  Extension alignments are refused on the register route for every scoring of the long world ("reads of
# more than 1024 rows") and for 150 x 600 ("cells could leave int16"), whatever extend_wide says -- but under band_width > 0 with
# extend_band = extend_band_align = 1 they run BANDED "whatever the read length, score_width (0 or 32) or extend_wide say", so
# every (world, scoring) has a state in which they succeed.  Spanned CIGARs are refused where spanned scores are, "and whatever
# the alignment route of the window's shape refuses": an unbanded Smith-Waterman alignment under traceback_policy = 0 picks its
# own cells and refuses nothing.)


def extension_route(state, family):
    """The route include/valign_hip.h gives a call of an extension family ("extend": the scores, "extend_align": the alignments)
    in this state, as far as the two band keys decide it -- a pure function of the state:
      "band" ...... the banded int32 strip sweep: the scores iff band_width > 0 and extend_band == 1, the alignments iff, in
                    addition, extend_band_align == 1.  (The route still refuses score_width = 16, traceback_policy = 1 and the NW
                    mode bit, with texts of its own: a refused call has run on no route.)
      "unbanded" .. band_width == 0: neither key is read; the register sweep, the int32 sweep of extend_wide, or their refusals.
      "refused" ... band_width > 0 and the family's keys are not all on: every call is refused for the band."""
    if family not in ("extend", "extend_align"):
        raise ValueError(family)
    if state["band_width"] == 0:
        return "unbanded"
    if state["extend_band"] == 1 and (family == "extend" or state["extend_band_align"] == 1):
        return "band"
    return "refused"


def capped_families(world):
    """The families whose calls a sequence of this world holds to SUBOPT_CALLS in its drawn part: the suboptimal scores, as ever,
    and every family that some scoring of the world refuses whatever the keys say."""
    out = {"subopt"}
    for scoring in WORLDS[world]["scorings"]:
        never = set(NEVER_SUCCEEDS.get((world, scoring), ()))
        out |= {f for f in FAMILIES if set(ENTRIES_OF[f]) <= never}
    return out


def key_values(world, key):
    """Every value the key takes in this world's sequences (the default among them, but for the set-only keys)."""
    if key == "band_width":
        return (0,) + tuple(WORLDS[world]["bands"])
    if key == "score_width":
        return (0, 16, 32)
    if key == "ragged_batching":
        return (0, 1, 2)
    if key == "pointer_scratch_cap_mb":
        return (2, 64)
    return (0, 1)


def initial_state():
    return dict(DEFAULTS)


def apply_step(state, step):
    """The state after a key-change step (a new dict); a call leaves it alone."""
    if step["kind"] != "set":
        return state
    if step["key"] in SET_ONLY_POSITIVE and step["value"] <= 0:
        raise ValueError("%s can only be set to a positive value" % step["key"])
    out = dict(state)
    out[step["key"]] = step["value"]
    return out


def configure(engine, state):
    """Apply a whole state to a new engine, key by key in the order of KEYS."""
    for key in KEYS:
        if key in SET_ONLY_POSITIVE and state[key] == 0:
            continue                        # never set: the engine's own default
        getattr(engine, "set_" + key)(state[key])


def pairs(world):
    """The world's pairs: mutated copies with indels, N runs, truncated (NUL-padded) pairs, lower case and junk bytes."""
    return _pairs(world)


@functools.lru_cache(maxsize=None)
def _pairs(world):
    w = WORLDS[world]
    reads, refs = synth.make_pairs(POOL, w["R"], w["F"], seed=1000 + 7 * w["R"] + w["F"], sub_rate=0.1, indel_rate=0.03, n_run_frac=0.1,
                                   short_frac=0.25, lowercase_frac=0.05, junk_frac=0.05)
    reads.setflags(write=False)
    refs.setflags(write=False)
    return reads, refs


# ---- the generator ----------------------------------------------------------------------------------------------------------
class _Draw:
    def __init__(self, world, seed):
        self.r = synth._stream(7000 + int(seed), _STREAM_OF[world], (8192,))
        self.k = 0

    def pick(self, lo, hi):
        v = int(lo + int(self.r[self.k] % np.uint64(hi - lo + 1)))
        self.k += 1
        return v

    def choice(self, items):
        return items[self.pick(0, len(items) - 1)]


def _blockers(world, state, family, alg):
    """What, by the header's refusal rules, stands between this state and a call of the family -- a list of alternative
    single-key remedies for the first reason found, [] when nothing does or nothing helps.  Only steers the generator (so that
    sequences are not mostly refusals); the tests never read it.  The short world is judged as if its scoring were the wide one.
    Spanned CIGARs are steered as spanned scores are: the window's alignment refuses nothing of its own here.  The two extension
    families are steered by extension_route(): under a band towards their keys or away from the band, and from band_width = 0
    towards a band of the world wherever only the Band route can run the call (the long world, the wide scoring)."""
    band, wide_scoring = state["band_width"], world == "short"
    if family in ("placed", "span", "subopt", "span_cigar", "extend", "extend_align") and alg == NW:
        return []
    if family in ("extend", "extend_align"):           # band_placed and placed_wide are not read
        bands = [("band_width", b) for b in WORLDS[world]["bands"]]
        if state["traceback_policy"]:
            return [("traceback_policy", 0)]
        route = extension_route(state, family)
        if route == "band":                             # whatever the read length, score_width 0 / 32 and extend_wide say
            return [("score_width", 0)] if state["score_width"] == 16 else []
        if route == "refused":                          # under a band: the family's keys, one at a time, or no band
            if not state["extend_band"]:
                return [("extend_band", 1), ("band_width", 0)]
            return [("extend_band_align", 1), ("band_width", 0)]
        if family == "extend_align":                    # no band: refused wherever the extension route would be wide -- the band route is what helps
            if world == "long":
                return bands
            if state["score_width"] == 32:
                return [("score_width", 0)] + bands
            return []                                   # (the register route serves every scoring but the wide one)
        if state["score_width"] == 32 and not state["extend_wide"]:
            return [("extend_wide", 1), ("score_width", 0)]
        if wide_scoring and state["score_width"] == 16:
            return [("score_width", 0)]
        if (wide_scoring or world == "long") and not state["extend_wide"]:
            return [("extend_wide", 1)] + bands[:1]
        return []
    if family == "score":
        if band > 0 and alg == NW and not state["band_nw"]:
            return [("band_nw", 1), ("band_width", 0)]
        if band == 0 and wide_scoring and state["score_width"] == 16:
            return [("score_width", 0), ("score_width", 32)]
        return []
    if family in ("rows", "cigar"):
        if band > 0 and state["band_alignments"]:
            if alg == NW and not state["band_nw"]:
                return [("band_nw", 1), ("band_alignments", 0)]
            if state["traceback_policy"]:
                return [("traceback_policy", 0), ("band_alignments", 0)]
        return []
    if band > 0:
        if family != "placed":
            return [("band_width", 0)]
        if not state["band_placed"]:
            return [("band_placed", 1), ("band_width", 0)]
        return [("traceback_policy", 0)] if state["traceback_policy"] else []
    if state["traceback_policy"]:
        return [("traceback_policy", 0)]
    if family == "subopt":
        return [("score_width", 0)] if state["score_width"] == 32 else []
    if state["score_width"] == 32 and not state["placed_wide"]:
        return [("placed_wide", 1), ("score_width", 0)]
    if wide_scoring and state["score_width"] == 16:
        return [("score_width", 0)]
    if wide_scoring and not state["placed_wide"]:
        return [("placed_wide", 1)]
    return []


def sequence(world, seed):
    """-> the steps of (world, seed): dicts {"kind": "set", "key", "value"} and {"kind": "call", "entry", "alg", "begin", "n",
    "threads", "mask", "extended", "end_bonus", "with_extend"}.  A pure function of its arguments."""
    w = WORLDS[world]
    d = _Draw(world, seed)
    state = initial_state()
    history = {k: [state[k]] for k in KEYS}
    steps, seen, count, likely = [], set(), {e: 0 for e in ENTRY_POINTS}, {e: 0 for e in ENTRY_POINTS}
    likely_band = {e: 0 for f in ("extend", "extend_align") for e in ENTRIES_OF[f]}        # ... of which on the Band route
    likely_unbanded = dict(likely_band)                                                     # ... and without a band
    made = []                           # (family, the state it was made in, the step) of every call so far
    capped = capped_families(world)
    last_family = None

    def change(key, value):
        nonlocal state
        if value == state[key]:
            return
        step = {"kind": "set", "key": key, "value": value}
        state = apply_step(state, step)
        history[key].append(value)
        steps.append(step)

    def call(family, alg=None, entry=None, remedy=False, as_it_is=False, **fixed):
        nonlocal last_family
        a, b = ENTRIES_OF[family]
        if entry is None:
            entry = a if count[a] < count[b] else b if count[b] < count[a] else d.choice((a, b))
        if alg is None:
            alg = d.choice((SW, NW)) if family in ("score", "rows", "cigar") else (NW if d.pick(0, 11) == 0 else SW)
        if not as_it_is and _blockers(world, state, family, alg) and (remedy or d.pick(0, 7)):
            # seven times in eight: remedy reason after reason, then call.  Five reasons at the most: traceback_policy, the band,
            # extend_band, extend_band_align, score_width
            for _ in range(5):
                fixes = _blockers(world, state, family, alg)
                if not fixes:
                    break
                change(*d.choice(fixes))
        # (for the repairs below; an affine scoring also refuses the register routes' alignments under traceback_policy = 1)
        if not _blockers(world, state, family, alg) and (family == "score" or alg == SW) and \
                (family not in ("rows", "cigar") or not state["traceback_policy"]):
            likely[entry] += 1
            if entry in likely_band and extension_route(state, family) == "band":
                likely_band[entry] += 1
            if entry in likely_band and extension_route(state, family) == "unbanded":
                likely_unbanded[entry] += 1
        n = d.choice(LADDER)
        step = {"kind": "call", "entry": entry, "alg": alg, "begin": d.pick(0, POOL - n), "n": n, "threads": d.pick(1, 3),
                "mask": d.choice((0, 3, w["R"] // 2, w["F"])), "extended": d.pick(0, 1), "end_bonus": d.choice(END_BONUSES),
                "with_extend": d.pick(0, 1)}
        step.update(fixed)
        steps.append(step)
        made.append((family, state, step))
        count[entry] += 1
        if last_family is not None:
            seen.add((last_family, family))
        last_family = family

    def family_calls(family):
        return sum(count[e] for e in ENTRIES_OF[family])

    for _ in range(CALLS):
        for _ in range(d.pick(0, 2)):
            key = d.choice(KEYS)
            change(key, d.choice([v for v in key_values(world, key) if v != state[key]]))
        open_families = [f for f in FAMILIES if f not in capped or family_calls(f) < SUBOPT_CALLS]
        fresh = [f for f in open_families if f != last_family and (last_family, f) not in seen]
        call(d.choice(fresh or open_families))
    # repairs: what the draw above did not bring about by itself
    for key in KEYS:
        values, h = key_values(world, key), history[key]
        while len(set(h)) < 2 or not any(h[i] in h[:i - 1] for i in range(2, len(h))):
            change(key, d.choice([v for v in values if v != state[key] and (len(h) < 2 or v in h[:-1])] or
                                 [v for v in values if v != state[key]]))
            call("score")
    for entry in ENTRY_POINTS:
        while count[entry] < 3:
            call(FAMILY_OF[entry], entry=entry)
        while likely[entry] < 3:                # by the steering model: calls that should run, so that no entry point hides behind refusals
            if FAMILY_OF[entry] in ("rows", "cigar"):
                change("traceback_policy", 0)
            call(FAMILY_OF[entry], alg=SW, entry=entry, remedy=True)
    # ... every value of the fields that only the new CIGAR families read
    for family, field, values in (("extend_align", "end_bonus", END_BONUSES), ("extend_align", "with_extend", (0, 1)),
                                  ("span_cigar", "extended", (0, 1))):
        for value in values:
            if not any(f == family and step[field] == value for f, _, step in made):
                call(family, alg=SW, remedy=True, **{field: value})
    # ... the orders in which two families use ONE piece of the engine: the spanned calls' child engine, the CIGAR calls' rows
    # scratch at its two pitches, the strip scratch of the two int32 sweeps
    for order in (("span", "span_cigar", "span"), ("cigar", "extend_align", "cigar")):
        families = [f for f, _, _ in made]
        if not any(tuple(families[i:i + 3]) == order for i in range(len(families) - 2)):
            for family in order:
                call(family, alg=SW, remedy=True)
    if not wide_sweeps_are_neighbours(made):
        change("placed_wide", 1)
        change("extend_wide", 1)
        call("placed", alg=SW, remedy=True)
        call("extend", alg=SW, remedy=True)
    # ... the state the Band route of the two extension families shares (module docstring); every call below is made as_it_is, in
    # a state set up so that the model expects it to run
    bands = w["bands"]

    def on_band(width):
        """the keys under which both extension families run BANDED, under the band `width`"""
        change("traceback_policy", 0)
        if state["score_width"] == 16:
            change("score_width", 0)
        change("extend_band", 1)
        change("extend_band_align", 1)
        change("band_width", width)

    # the strip scratch under three layouts: the placed int32 sweep, banded extension scores, banded extension alignments --
    # pairwise neighbours in both orders
    if not STRIP_SCRATCH_ORDERS <= strip_scratch_neighbours(made):
        band = state["band_width"] or bands[0]
        change("placed_wide", 1)
        change("score_width", 32)
        for family in ("placed", "extend", "extend_align", "placed", "extend_align", "extend", "placed"):
            on_band(0 if family == "placed" else band)
            call(family, alg=SW, as_it_is=True)
    # the pointer scratch and the rows scratch at two pitches: unbanded CIGARs around a banded extension alignment
    if not pointer_scratch_order(made):
        on_band(state["band_width"] or bands[1])
        change("band_alignments", 0)
        for family in ("cigar", "extend_align", "cigar"):
            call(family, alg=SW, as_it_is=True)
    # the pointer layout of the band at two w: one band, the other, the first again
    if not two_bands_order(made):
        for width in (bands[0], bands[1], bands[0]):
            on_band(width)
            call("extend_align", alg=SW, as_it_is=True)
    # a banded extension call directly before and after band_width goes to 0 and comes back: the register route in between (tiny)
    # or the routes extend_wide opens
    if not band_cleared_order(made):
        band = state["band_width"] or bands[1]
        on_band(band)
        call("extend", alg=SW, as_it_is=True)
        change("band_width", 0)
        if world == "tiny":
            change("score_width", 0)
            call("extend_align", alg=SW, as_it_is=True)
        else:
            change("extend_wide", 1)
            call("extend", alg=SW, as_it_is=True)
        on_band(band)
        call("extend_align", alg=SW, as_it_is=True)
    # every value of end_bonus and with_extend ON the Band route, every extension entry point there twice by the model, and both
    # families under a band with their keys off (refused: the text and the describe() of a new engine)
    for field, values in (("end_bonus", END_BONUSES), ("with_extend", (0, 1))):
        for value in values:
            if not any(f == "extend_align" and runs_banded(f, s, step) and step[field] == value for f, s, step in made):
                on_band(state["band_width"] or bands[0])
                call("extend_align", alg=SW, as_it_is=True, **{field: value})
    for entry in likely_band:
        while likely_band[entry] < 2:
            on_band(state["band_width"] or bands[1])
            call(FAMILY_OF[entry], alg=SW, entry=entry, as_it_is=True)
    # ... the routes without a band keep their share: every extension entry point twice by the model where a route without a band
    # can serve it (the scores everywhere, under extend_wide where need be; the alignments on the register route -- not in the long
    # world, where only the Band route runs them)
    for entry in likely_unbanded:
        family = FAMILY_OF[entry]
        while likely_unbanded[entry] < 2 and (family == "extend" or world != "long"):
            change("band_width", 0)
            change("traceback_policy", 0)
            if family == "extend_align" or state["score_width"] == 16:
                change("score_width", 0)
            if family == "extend":
                change("extend_wide", 1)
            call(family, alg=SW, entry=entry, as_it_is=True)
    off = {f for f, s, _ in made if f in ("extend", "extend_align") and extension_route(s, f) == "refused"}
    for family in ("extend", "extend_align"):
        if family not in off:
            change("band_width", state["band_width"] or bands[0])
            change("extend_band", 0)
            call(family, alg=SW, as_it_is=True)
    # ... and, always, a band that is set, used, cleared and followed by a call of every family that reads the plan
    change("band_width", w["bands"][0])
    call("score", alg=SW)
    change("band_width", 0)
    for family in ("score", "rows", "placed", "extend", "span_cigar"):
        call(family, alg=SW)
    return steps


def wide_sweeps_are_neighbours(made):
    """made: (family, state, step) per call, in order.  True where a placed call under placed_wide = 1 and an extension-score call
    under extend_wide = 1 follow one another, in either order: the two int32 sweeps on the one strip scratch."""
    def wide(family, state):
        return (family == "placed" and state["placed_wide"] == 1) or (family == "extend" and state["extend_wide"] == 1)
    return any(wide(fa, sa) and wide(fb, sb) and fa != fb for (fa, sa, _), (fb, sb, _) in zip(made, made[1:]))


def runs_banded(family, state, step):
    """The model's statement that this call runs on the Band route of its extension family: the route is "band" and nothing of what
    that route refuses stands in the way."""
    return (family in ("extend", "extend_align") and step["alg"] == SW and extension_route(state, family) == "band"
            and state["traceback_policy"] == 0 and state["score_width"] != 16)


def placed_on_int32(family, state, step):
    """a placed call that takes the int32 sweep whatever the world and the scoring: no band, score_width = 32 under placed_wide = 1"""
    return (family == "placed" and step["alg"] == SW and state["band_width"] == 0 and state["placed_wide"] == 1
            and state["score_width"] == 32 and state["traceback_policy"] == 0)


STRIP_SCRATCH_ORDERS = frozenset((a, b) for a in ("placed", "extend", "extend_align") for b in ("placed", "extend", "extend_align") if a != b)


def strip_scratch_neighbours(made):
    """made: (family, state, step) per call, in order -> the ordered pairs of ("placed", "extend", "extend_align") that follow one
    another as a placed call on its int32 sweep, a banded extension score and a banded extension alignment: the strip scratch
    (Engine::d_placed_rows_ / d_placed_ends_) under its three record layouts."""
    def kind(family, state, step):
        if placed_on_int32(family, state, step):
            return "placed"
        return family if runs_banded(family, state, step) else None
    kinds = [kind(*m) for m in made]
    return {(a, b) for a, b in zip(kinds, kinds[1:]) if a and b and a != b}


def _triples(made):
    return zip(made, made[1:], made[2:])


def pointer_scratch_order(made):
    """True where an unbanded CIGAR call, a banded extension alignment and an unbanded CIGAR call follow one another: the pointer
    scratch of every alignment fill, and the CIGAR rows scratch at the pitches R + F and R + F + 1."""
    def unbanded_cigar(family, state, step):
        return family == "cigar" and (state["band_width"] == 0 or state["band_alignments"] == 0)
    return any(unbanded_cigar(*a) and b[0] == "extend_align" and runs_banded(*b) and unbanded_cigar(*c) for a, b, c in _triples(made))


def two_bands_order(made):
    """True where three banded extension alignments follow one another under one band, another, and the first again."""
    return any(all(m[0] == "extend_align" and runs_banded(*m) for m in (a, b, c)) and a[1]["band_width"] == c[1]["band_width"] != b[1]["band_width"]
               for a, b, c in _triples(made))


def band_cleared_order(made):
    """True where a banded extension call, an extension call under band_width = 0 and a banded extension call follow one another."""
    return any(runs_banded(*a) and b[0] in ("extend", "extend_align") and b[2]["alg"] == SW and b[1]["band_width"] == 0 and runs_banded(*c)
               for a, b, c in _triples(made))


def calls_with_state(steps):
    """-> (family, the state the call is made in, the step) of every call of `steps`, in order"""
    out, state = [], initial_state()
    for step in steps:
        state = apply_step(state, step)
        if step["kind"] == "call":
            out.append((FAMILY_OF[step["entry"]], state, step))
    return out


# ---- the runner -------------------------------------------------------------------------------------------------------------
ECHOED = ("band_width", "ragged_batching", "band_alignments", "band_nw", "band_placed", "placed_wide", "extend_wide", "extend_band",
          "extend_band_align", "trace_checkpoints")
PLAN_KEYS = ("long_mode", "group_lanes", "rows_per_lane", "score_cells", "band_block_rows", "band_col_align", "span_ref_length",
             "extend_band_block_rows")
RAN_KEYS = {"score": ("ran_score_cells", "ran_score_geometry", "ran_score_sym_affine"),
            "rows": ("ran_align_fill", "ran_align_geometry", "ran_result_format"),
            "cigar": ("ran_align_fill", "ran_align_geometry", "ran_result_format", "ran_cigar_lanes"),
            "placed": ("ran_placed", "ran_placed_geometry"), "span": ("ran_span", "ran_placed", "ran_placed_geometry"),
            "subopt": ("ran_subopt", "ran_subopt_geometry"),
            "span_cigar": ("ran_span_cigar", "ran_placed", "ran_placed_geometry", "ran_result_format", "ran_cigar_lanes"),
            "extend": ("ran_extend", "ran_extend_geometry"),
            "extend_align": ("ran_extend_align", "ran_extend_align_geometry", "ran_cigar_lanes")}
SENTINEL = -7


class SequenceMismatch(AssertionError):
    pass


def compared(entry, desc, refused=False):
    """The describe() keys a live engine and a new one must agree on right after a call of `entry` (a key the library leaves
    out -- ran_score_sym_affine -- reads None).  Scratch sizes and the last-launch figures of other kinds of call are not here:
    direct_call, packed_classes and ragged_launches are figures of the last host-pointer / score call that LAUNCHED, so after a
    refused call they are an earlier call's and are left out.  After an extension alignment that ran, align_ptr_bytes_per_pair is
    the call's own -- on the Band route a function of state and shape alone -- and is compared.  ran_extend_align_chunks is NOT:
    the chunk size reads hipMemGetInfo, and a live engine that holds scratch sees other free memory than a new one."""
    family = FAMILY_OF[entry]
    out = {k: desc.get(k) for k in PLAN_KEYS + ECHOED + RAN_KEYS[family]}
    if family == "extend_align" and not refused:
        out["align_ptr_bytes_per_pair"] = desc["align_ptr_bytes_per_pair"]
    if entry.endswith("_host") and not refused:
        out["direct_call"] = desc["direct_call"]
        out["packed_classes"] = desc["packed_classes"]
    if family == "score" and not refused:
        out["ragged_launches_zero"] = desc["ragged_launches"] == 0
    return out


def _freeze(step):
    return tuple(sorted(step.items()))


class Runner:
    """One (world, scoring): the pairs on the device, the references (computed once per operation and parameter set, for the
    whole pool, and sliced), and run(seed_or_steps).  device=False: the part that only compares -- the references, expected() and
    verify() -- without torch and without a GPU (tests/test_engine_sequences.py holds verify() to two mutants there)."""

    def __init__(self, world, scoring, device=True):
        from oracle import cpu_ref
        from versalignlib_amd import hipkernel
        self.torch, self.cpu_ref, self.hk = None, cpu_ref, hipkernel
        self.world, self.scoring = world, scoring
        w = WORLDS[world]
        self.R, self.F = w["R"], w["F"]
        self.args = SCORINGS[scoring]
        self.affine = len(self.args) > 4
        self.osc = cpu_ref.Scoring.make(*self.args)
        self.hsc = hipkernel.Scoring.make(*self.args)
        self.reads, self.refs = pairs(world)
        if device:
            import torch
            self.torch = torch
            self.d_reads = torch.from_numpy(np.array(self.reads)).cuda()
            self.d_refs = torch.from_numpy(np.array(self.refs)).cuda()
        self.stride = self.R + self.F           # ops per pair of the device-resident CIGAR calls: no alignment has more
        self._refs = {}

    # -- references: the whole pool, once --
    def _ref(self, key, make):
        if key not in self._refs:
            out = make()
            for a in (out if isinstance(out, tuple) else (out,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._refs[key] = out
        return self._refs[key]

    def ref_scores(self, alg, band, block):
        import band_nw_ref
        if band == 0:
            return self._ref(("score", alg), lambda: self.cpu_ref.score(alg, self.reads, self.refs, self.osc, threads=8, affine=self.affine, wide=True))
        if alg == SW:
            return self._ref(("score", alg, band, block), lambda: self.cpu_ref.score_banded_sw(
                self.reads, self.refs, band, self.osc, threads=8, block_rows=block[0], col_align=block[1], affine=self.affine))
        return self._ref(("score", alg, band, block), lambda: np.minimum(band_nw_ref.score_banded_nw(
            self.reads, self.refs, band, self.osc, block_rows=block[0], col_align=block[1], affine=self.affine), 32767).astype(np.int16))

    def ref_rows(self, alg, band, block, policy, wide):
        import band_align_ref
        import band_nw_ref
        if band == 0:
            return self._ref(("rows", alg, policy, wide), lambda: self.cpu_ref.align(
                alg, self.reads, self.refs, self.osc, threads=8, affine=self.affine, policy="sse" if policy else "default", wide=wide))
        fn = band_align_ref.align_banded_sw if alg == SW else band_nw_ref.align_banded_nw
        return self._ref(("rows", alg, band, block), lambda: fn(self.reads, self.refs, band, self.osc, block_rows=block[0], col_align=block[1],
                                                                affine=self.affine))

    def ref_cigar(self, rows_key, rows, idx, extended):
        import cigar_ref
        return self._ref(("cigar", rows_key, extended), lambda: cigar_ref.expected(np.array(rows), np.array(idx), self.osc, self.reads, self.refs,
                                                                                   extended=bool(extended), affine=self.affine))

    def ref_placed(self, band):
        import placed_band_ref
        import placed_ref
        if band == 0:
            return self._ref(("placed",), lambda: placed_ref.placed(self.reads, self.refs, self.hsc, affine=self.affine))
        return self._ref(("placed", band), lambda: placed_band_ref.placed_banded(self.reads, self.refs, band, self.hsc, affine=self.affine))

    def ref_span(self):
        import span_ref
        return self._ref(("span",), lambda: span_ref.spans(self.reads, self.refs, self.hsc, affine=self.affine))

    def ref_span_cigar(self, extended):
        import span_cigar_ref
        return self._ref(("span_cigar", extended), lambda: span_cigar_ref.expected(self.reads, self.refs, self.hsc, affine=self.affine,
                                                                                   extended=bool(extended)))

    def ref_extend(self):
        """one reference for both routes: the record is the same on the register sweep and on the int32 sweep"""
        import extend_ref
        return self._ref(("extend",), lambda: extend_ref.extend(self.reads, self.refs, self.hsc, self.affine))

    def ref_extend_align(self, extended):
        """-> {end_bonus: (recs, ops, extension records, end cells)}: every bonus from ONE fill of the matrices"""
        import extend_align_ref
        return self._ref(("extend_align", extended), lambda: dict(zip(END_BONUSES, extend_align_ref.align(
            self.reads, self.refs, self.hsc, self.affine, end_bonus=END_BONUSES, extended=bool(extended)))))

    def ref_extend_band(self, band):
        """the Band route's records: the cells outside the band on the anchor's diagonal are absent, an unreached read end is
        VALIGN_HIP_EXTEND_UNREACHED"""
        import extend_band_ref
        return self._ref(("extend_band", band), lambda: extend_band_ref.extend(self.reads, self.refs, self.hsc, band, self.affine))

    def ref_extend_band_align(self, band, extended):
        """-> {end_bonus: (recs, ops, extension records, end cells, paths)}: every bonus from ONE fill per (band, extended)"""
        import extend_band_align_ref
        return self._ref(("extend_band_align", band, extended), lambda: dict(zip(END_BONUSES, extend_band_align_ref.align(
            self.reads, self.refs, self.hsc, band, self.affine, end_bonus=END_BONUSES, extended=bool(extended)))))

    def ref_subopt(self, mask):
        import subopt_ref
        prepared = self._ref(("subopt",), lambda: subopt_ref.prepare(self.reads, self.refs, self.hsc, affine=self.affine))
        return self._ref(("subopt", mask), lambda: subopt_ref.apply_mask(prepared, mask))

    # -- one call on one engine --
    def outputs(self, step, stream=None):
        """Preallocated, sentinel-filled outputs of a device-resident call (None for a host call); the fill is queued on
        `stream`, in front of the call that follows there."""
        t, n, entry = self.torch, step["n"], step["entry"]

        def full(shape, dtype):
            with t.cuda.stream(stream):
                return t.full(shape, SENTINEL, dtype=dtype, device="cuda")
        if entry == "score_device":
            return (full((n,), t.int16),)
        if entry == "align_device":
            return (full((n, 2, self.R + self.F), t.uint8), full((n, 4), t.int16))
        if entry == "align_cigar_device":
            return (full((n, 6), t.int32), full((n, self.stride), t.int32))
        if entry == "score_placed_device":
            return (full((n, 3), t.int32),)
        if entry in ("score_span_device", "score_subopt_device", "score_extend_device"):
            return (full((n, 5), t.int32),)
        if entry == "align_span_device":
            return (full((n, 6), t.int32), full((n, self.stride), t.int32))
        if entry == "align_extend_device":         # ... and the extension records only where the call asks for them
            return (full((n, 6), t.int32), full((n, self.stride), t.int32)) + ((full((n, 5), t.int32),) if step["with_extend"] else ())
        return None

    def issue(self, eng, step, out, stream):
        """Make the call.  -> ("ok", result) -- a device call's result is `out`, still in flight on `stream` -- or
        ("refused", message).  Nothing here waits for the stream."""
        b, e, alg, entry = step["begin"], step["begin"] + step["n"], step["alg"], step["entry"]
        dr, df, hr, hf = self.d_reads[b:e], self.d_refs[b:e], self.reads[b:e], self.refs[b:e]
        try:
            if entry == "score_device":
                eng.score_device(alg, dr, df, scores=out[0], stream=stream)
            elif entry == "align_device":
                eng.align_device(alg, dr, df, rows=out[0], idx=out[1], stream=stream)
            elif entry == "align_cigar_device":
                eng.align_cigar_device(alg, dr, df, extended=bool(step["extended"]), ops_stride=self.stride, stream=stream, out=out)
            elif entry == "score_placed_device":
                eng.score_placed_device(alg, dr, df, out=out[0], stream=stream)
            elif entry == "score_span_device":
                eng.score_span_device(alg, dr, df, out=out[0], stream=stream)
            elif entry == "score_subopt_device":
                eng.score_subopt_device(alg, dr, df, step["mask"], out=out[0], stream=stream)
            elif entry == "align_span_device":
                eng.align_span_device(alg, dr, df, extended=bool(step["extended"]), ops_stride=self.stride, stream=stream, out=out)
            elif entry == "score_extend_device":
                eng.score_extend_device(alg, dr, df, out=out[0], stream=stream)
            elif entry == "align_extend_device":
                back = eng.align_extend_device(alg, dr, df, end_bonus=step["end_bonus"], extended=bool(step["extended"]), ops_stride=self.stride,
                                               with_extend=bool(step["with_extend"]), stream=stream, out=out if step["with_extend"] else out + (None,))
                assert step["with_extend"] or back[2] is None, "extension records nobody asked for"
            elif entry == "align_span_host":
                out = eng.align_span_host(alg, hr, hf, extended=bool(step["extended"]), threads=step["threads"])
            elif entry == "score_extend_host":
                out = (eng.score_extend_host(alg, hr, hf, threads=step["threads"]),)
            elif entry == "align_extend_host":
                out = eng.align_extend_host(alg, hr, hf, end_bonus=step["end_bonus"], extended=bool(step["extended"]),
                                            with_extend=bool(step["with_extend"]), threads=step["threads"])
                if not step["with_extend"]:
                    assert out[3] is None, "extension records nobody asked for"
                    out = out[:3]
            elif entry == "score_host":
                out = (eng.score_host(alg, hr, hf, threads=step["threads"]),)
            elif entry == "align_host":
                out = eng.align_host(alg, hr, hf, threads=step["threads"])
            elif entry == "align_cigar_host":
                out = eng.align_cigar_host(alg, hr, hf, extended=bool(step["extended"]), threads=step["threads"])
            elif entry == "score_placed_host":
                out = (eng.score_placed_host(alg, hr, hf, threads=step["threads"]),)
            elif entry == "score_span_host":
                out = (eng.score_span_host(alg, hr, hf, threads=step["threads"]),)
            elif entry == "score_subopt_host":
                out = (eng.score_subopt_host(alg, hr, hf, step["mask"], threads=step["threads"]),)
            else:
                raise ValueError(entry)
        except self.hk.HipKernelError as err:
            return "refused", str(err)
        return "ok", out

    @staticmethod
    def landed(out):
        """The result as numpy arrays, once the stream is through."""
        return tuple(a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a) for a in out)

    def fresh(self, state, step, cache):
        """What a NEW engine configured to `state` returns for the call: (outcome, arrays or message, compared describe keys)."""
        key = (tuple(state[k] for k in KEYS), _freeze(step))
        if key not in cache:
            eng = self.hk.Engine(self.R, self.F, self.hsc)
            try:
                configure(eng, state)
                out = self.outputs(step)
                outcome, res = self.issue(eng, step, out, None)
                self.torch.cuda.synchronize()
                desc = compared(step["entry"], eng.describe(step["alg"], step["n"]), outcome == "refused")
                cache[key] = (outcome, self.landed(res) if outcome == "ok" else res, desc)
            finally:
                eng.close()
        return cache[key]

    # -- the reference of a successful call --
    def expected(self, state, step, desc):
        """The arrays the call must have returned, in the entry point's own layout, from the reference of the operation the
        state selects (include/valign_hip.h says which); desc: the live engine's describe() right after the call."""
        b, e, alg, family = step["begin"], step["begin"] + step["n"], step["alg"], FAMILY_OF[step["entry"]]
        band = state["band_width"]
        block = (desc["band_block_rows"], desc["band_col_align"])
        if family == "score":
            return (self.ref_scores(alg, band, block)[b:e],)
        if family in ("rows", "cigar"):
            banded = band > 0 and state["band_alignments"]
            fill = desc["ran_align_fill"]
            # the cell width of the expected alignments is the one that ran, never "either": strip_wide* is the oracle's wide=True
            wide = fill.startswith("strip_wide")
            key = ("rows", alg, band, block) if banded else ("rows", alg, state["traceback_policy"], wide)
            rows, idx = self.ref_rows(alg, band if banded else 0, block, state["traceback_policy"], wide)
            if family == "rows":
                return rows[b:e], idx[b:e]
            exp = self.ref_cigar(key, rows, idx, step["extended"])
            return {k: v[b:e] for k, v in exp.items()}
        if family == "placed":
            return (self.ref_placed(band)[b:e],)
        if family == "span":
            return (self.ref_span()[b:e],)
        if family == "span_cigar":
            exp = self.ref_span_cigar(step["extended"])
            return exp["recs"][b:e], exp["ops"][b:e], None
        if family in ("extend", "extend_align"):
            # the route that ran must be the one the rule names, before any reference is picked: a call that quietly took another
            # route is not judged against that route's reference
            ran = "ran_extend" if family == "extend" else "ran_extend_align"
            route = extension_route(state, family)
            if route == "refused" or (desc[ran] == "band") != (route == "band") or (route == "band" and desc[ran + "_geometry"] != "none"):
                raise SequenceMismatch(("the extension route", route, "by include/valign_hip.h, but describe() says", ran, desc[ran],
                                        ran + "_geometry", desc[ran + "_geometry"], "state", state))
            banded = route == "band"
            # (the extension records of an alignment call are the SCORE call's, bit for bit -- UNREACHED included under a band)
            scores = self.ref_extend_band(band) if banded else self.ref_extend()
            if family == "extend":
                return (scores[b:e],)
            res = (self.ref_extend_band_align(band, step["extended"]) if banded else self.ref_extend_align(step["extended"]))[step["end_bonus"]]
            return res[0][b:e], res[1][b:e], scores[b:e] if step["with_extend"] else None
        return (self.ref_subopt(step["mask"])[b:e],)

    def verify(self, step, got, exp, where):
        import cigar_ref
        entry, family = step["entry"], FAMILY_OF[step["entry"]]
        b, e = step["begin"], step["begin"] + step["n"]
        if family == "cigar":
            if entry.endswith("_device"):
                recs = got[0].view(self.hk.aln_dtype()).reshape(-1)
                ops = got[1].view(np.uint32)
                assert (recs["n_ops"] <= self.stride).all(), (where, "n_ops beyond the stride")
                cigar_ref.check(recs, lambda p: ops[p, :recs["n_ops"][p]], exp, self.reads[b:e], self.refs[b:e], where)
                tail = np.arange(self.stride)[None, :] >= recs["n_ops"][:, None].astype(np.int64)
                assert (got[1][tail] == SENTINEL).all(), (where, "words past a pair's ops were written")
            else:
                recs, ops, offsets = got
                assert offsets[0] == 0 and np.array_equal(np.diff(offsets), recs["n_ops"].astype(np.int64)) and len(ops) == offsets[-1], (where, "offsets")
                cigar_ref.check(recs, lambda p: ops[offsets[p]:offsets[p + 1]], exp, self.reads[b:e], self.refs[b:e], where)
            return
        if family in ("span_cigar", "extend_align"):
            self._verify_compact(entry, got, exp, where)
            return
        if entry.endswith("_host") and family in ("placed", "span", "subopt", "extend"):
            got = (np.stack([got[0][k] for k in got[0].dtype.names], axis=1),)
        for g, x in zip(got, exp):
            g, x = np.asarray(g), np.asarray(x)
            same = g.astype(np.int64) == x.astype(np.int64)
            if not same.all():
                bad = np.nonzero(~same.reshape(len(g), -1).all(axis=1))[0]
                raise SequenceMismatch((where, "differs from the reference at pairs", bad[:6].tolist(), "got", g[bad[:2]].tolist()[:2],
                                        "expected", x[bad[:2]].tolist()[:2]))

    def _verify_compact(self, entry, got, exp, where):
        """Spanned CIGARs and extension alignments, exactly (test_gpu_span_cigar._check, test_gpu_extend_align._check): every
        record field, every op of every pair, the sentinel behind a pair's ops (device) or the offsets (host), and the extension
        records where the call asked for them -- no buffer of them where it did not."""
        exp_recs, exp_ops, exp_ext = exp
        n = len(exp_recs)
        if entry.endswith("_device"):
            recs, ext = got[0].astype(np.int64), got[2] if len(got) > 2 else None
            ops = got[1].view(np.uint32)
            if not (recs[:, 5] <= self.stride).all():
                raise SequenceMismatch((where, "n_ops beyond the stride", int(recs[:, 5].max()), self.stride))

            def ops_of(p):
                return ops[p, :recs[p, 5]]
            tail = np.arange(self.stride)[None, :] >= recs[:, 5][:, None]
            if not (got[1][tail] == SENTINEL).all():
                raise SequenceMismatch((where, "words past a pair's ops were written, at pairs",
                                        np.nonzero(((got[1] != SENTINEL) & tail).any(axis=1))[0][:6].tolist()))
        else:
            recs = np.stack([got[0][k] for k in self.hk.aln_dtype().names], axis=1).astype(np.int64)
            ops, offsets, ext = got[1], got[2], got[3] if len(got) > 3 else None
            if ext is not None:
                ext = np.stack([ext[k] for k in self.hk.extend_dtype().names], axis=1)
            if not (len(offsets) == n + 1 and offsets[0] == 0 and np.array_equal(np.diff(offsets), recs[:, 5]) and len(ops) == offsets[-1]):
                raise SequenceMismatch((where, "offsets", offsets[:8].tolist(), recs[:8, 5].tolist(), len(ops)))

            def ops_of(p):
                return ops[offsets[p]:offsets[p + 1]]
        bad = np.nonzero((recs != exp_recs).any(axis=1))[0]
        if bad.size:
            raise SequenceMismatch((where, "records differ from the reference at pairs", bad[:6].tolist(), "got", recs[bad[:2]].tolist(),
                                    "expected", exp_recs[bad[:2]].tolist()))
        for p in range(n):
            want = [int(o) for o in exp_ops[p]]
            if [int(o) for o in ops_of(p)] != want:
                raise SequenceMismatch((where, "ops differ from the reference at pair", p, [int(o) for o in ops_of(p)][:12], want[:12]))
        if (ext is None) != (exp_ext is None):
            raise SequenceMismatch((where, "extension records", "missing" if ext is None else "returned though with_extend = 0"))
        if ext is not None:
            bad = np.nonzero((ext.astype(np.int64) != exp_ext).any(axis=1))[0]
            if bad.size:
                raise SequenceMismatch((where, "extension records differ from the reference at pairs", bad[:6].tolist(), "got", ext[bad[:2]].tolist(),
                                        "expected", exp_ext[bad[:2]].tolist()))

    # -- the whole sequence on one engine --
    def run(self, seed=None, steps=None, log=None):
        """Run sequence(world, seed) -- or `steps` -- on ONE engine.  Raises SequenceMismatch (an AssertionError) that names world,
        scoring, seed and step index.  -> {"calls", "refused", "succeeded": {entry: count}, "routes": {extension entry: {what
        ran_extend / ran_extend_align said after a call that ran: count}}, "chunks": {step index of an extension alignment that
        ran: the live engine's ran_extend_align_chunks}}."""
        torch = self.torch
        steps = sequence(self.world, seed) if steps is None else steps
        tag = (self.world, self.scoring, "seed", seed)
        # 1. the new engines first: each is created, configured, called once, waited for and closed (closing frees device
        #    memory, which waits for the device -- nothing of that may happen between the live engine's steps)
        cache, news, state = {}, {}, initial_state()
        for i, step in enumerate(steps):
            state = apply_step(state, step)
            if step["kind"] == "call":
                news[i] = (dict(state), self.fresh(state, step, cache))
        # 2. the live engine: one non-default stream, device steps back to back, a wait only before a host-pointer step and
        #    at the end.  describe() is host-side state and is read right after the call -- but where the very next step settles
        #    (a host-pointer call, or the end): nothing can change the state in between, so it is read in settle(), behind the
        #    wait.  After a score call on the 8 x 19 side tile describe() itself waits for the device (the module's docstring):
        #    read late, it costs a device step its place in the queue only where a key change or another device step follows.
        stream = torch.cuda.Stream()
        live = self.hk.Engine(self.R, self.F, self.hsc)
        pending, stats = [], {"calls": 0, "refused": 0, "succeeded": {e: 0 for e in ENTRY_POINTS},
                              "routes": {e: {} for f in ("extend", "extend_align") for e in ENTRIES_OF[f]}, "chunks": {}}

        def settles_next(i):
            return i + 1 == len(steps) or (steps[i + 1]["kind"] == "call" and steps[i + 1]["entry"].endswith("_host"))

        def settle():
            stream.synchronize()
            for i, step, outcome, res, desc in pending:
                if desc is None:            # (the last one pending: no step since)
                    assert i == pending[-1][0]
                    desc = live.describe(step["alg"], step["n"])
                self._settle(tag, i, step, outcome, res, desc, news[i])
                if outcome == "ok" and step["entry"] in stats["routes"]:       # the route of a call that ran and was verified
                    ran = desc["ran_extend" if FAMILY_OF[step["entry"]] == "extend" else "ran_extend_align"]
                    stats["routes"][step["entry"]][ran] = stats["routes"][step["entry"]].get(ran, 0) + 1
                    if FAMILY_OF[step["entry"]] == "extend_align":         # (the live engine's own figure: compared() says why it is not compared)
                        stats["chunks"][i] = desc["ran_extend_align_chunks"]
            del pending[:]

        try:
            for i, step in enumerate(steps):
                if step["kind"] == "set":
                    getattr(live, "set_" + step["key"])(step["value"])
                    continue
                if step["entry"].endswith("_host"):
                    settle()
                out = self.outputs(step, stream)
                outcome, res = self.issue(live, step, out, stream)
                desc = None if step["entry"].endswith("_device") and settles_next(i) else live.describe(step["alg"], step["n"])
                if log:
                    log("%4d %s %s -> %s %s" % (i, step["entry"], {k: v for k, v in step.items() if k not in ("kind", "entry")}, outcome,
                                                 res if outcome == "refused" else ""))
                stats["calls"] += 1
                if outcome == "ok":
                    stats["succeeded"][step["entry"]] += 1
                else:
                    stats["refused"] += 1
                pending.append((i, step, outcome, res if outcome == "ok" else (res, out), desc))
            settle()
        finally:
            stream.synchronize()
            live.close()
        return stats

    def _settle(self, tag, i, step, outcome, res, desc, fresh):
        where = tag + ("step", i, step["entry"], "alg", step["alg"], "pairs", (step["begin"], step["n"]))
        state, (f_outcome, f_res, f_desc) = fresh
        if outcome != f_outcome:
            raise SequenceMismatch((where, "live engine:", outcome, res[0] if outcome == "refused" else "", "new engine:", f_outcome,
                                    f_res if f_outcome == "refused" else "", "state", state))
        l_desc = compared(step["entry"], desc, outcome == "refused")
        if l_desc != f_desc:
            diff = {k: (l_desc[k], f_desc[k]) for k in l_desc if l_desc[k] != f_desc[k]}
            raise SequenceMismatch((where, "describe() of the live engine and of a new one differ (live, new)", diff, "state", state))
        if outcome == "refused":
            message, out = res
            if message != f_res:
                raise SequenceMismatch((where, "refused with another text", message, f_res))
            for a in (out or ()):
                if not bool((a == SENTINEL).all()):
                    raise SequenceMismatch((where, "a refused call wrote its output"))
            return
        got = self.landed(res)
        try:
            exp = self.expected(state, step, desc)
        except SequenceMismatch as err:                                       # (the route check: it does not know where it is)
            raise SequenceMismatch((where,) + tuple(err.args[0])) from None
        self.verify(step, got, exp, where)                                    # the authority: the reference, bit for bit
        for g, f in zip(got, f_res):                                          # ... and the new engine (unwritten words hold the sentinel in both)
            if not np.array_equal(g, f):
                raise SequenceMismatch((where, "live engine and new engine return different results", "state", state))
