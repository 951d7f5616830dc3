"""One engine through a whole sequence of key changes and calls (tests/engine_sequences.py), against the references and against
new engines.

Per (world, scoring, seed) ONE engine runs sequence(world, seed): device-resident calls go on one non-default stream into
preallocated, sentinel-filled outputs, back to back; the stream is waited for only before a host-pointer step and at the end
(the contract is one stream per engine).  describe() is host-side state and is read right after a call -- but for one key: after
a score call whose last launch ran on the 8 x 19 side tile, "ran_score_sym_affine_form" is read from the device, and
Engine::ran_side_tile_form waits for the whole device first.  (short, sym_affine) is that tile's window: a length-sorted score
call under half_float_cells = 0 takes it, and until another score call runs elsewhere every describe() of that engine drains the
stream.  The runner reads describe() behind its own wait wherever the very next step settles; elsewhere in those sequences the
device steps are not back to back.  Every call step is held against
  * the reference of the operation its state selects, bit for bit -- the authority: oracle/cpu_ref for unbanded scores and
    alignments (the cell width of an alignment read from ran_align_fill, never "either"), cpu_ref.score_banded_sw /
    band_align_ref / band_nw_ref under a band on the block shape describe() reports, cigar_ref, placed_ref / placed_band_ref,
    span_ref, subopt_ref, span_cigar_ref, extend_ref (one reference for the register sweep and the int32 sweep) and
    extend_align_ref -- and, where engine_sequences.extension_route() says "band", extend_band_ref and extend_band_align_ref,
    after asserting that ran_extend / ran_extend_align say "band" exactly there: a call that quietly took another route is not
    judged against that route's reference;
  * a NEW engine of the same shape and scoring, configured to the current state, that makes the same call on the same data:
    the same result or the same refusal with the same text, and the same describe() keys (engine_sequences.compared);
  * its own sentinel, where a device-resident call was refused.
A sequence must not hide behind refusals: at most a third of its calls end refused and every entry point succeeds at least
twice -- but for the suboptimal scores where include/valign_hip.h refuses them whatever the keys say
(engine_sequences.NEVER_SUCCEEDS: reads of more than 1 024 rows; a scoring whose cells leave int16).  Extension alignments are
no exception any more: in the long world and under the wide scoring the Band route runs them, and every extension entry point
must have run on that route at least twice in every sequence (the runner's per-route counts, read from ran_extend /
ran_extend_align).

Four hand-written sequences, one per piece of state that the newer entry points share with the older ones and with each other:
test_spanned_calls_share_one_child_engine, test_cigar_rows_scratch_at_two_pitches, test_int32_sweeps_share_the_strip_scratch,
test_extend_wide_flips_around_a_refusal.  Four more for the Band route of the extension families (extend_band,
extend_band_align), with exact call, refusal, per-entry and per-route counts: test_band_route_shares_the_strip_scratch (the strip
scratch of the placed int32 sweep, of extend_wide and of the placed strip route, at batch sizes that shrink to one pair and grow
again, device and host entries), test_band_route_shares_the_pointer_scratch (the pointer scratch in chunks under a 2 MB cap and
the CIGAR rows scratch at two pitches), test_two_bands_on_one_engine, test_extend_band_keys_flip_around_refusals.  Three of them
also run in the strips world (520 x 600, engine_sequences.WORLDS): a read that crosses a 512-row strip boundary and reaches its
end inside the band; its references take seconds each on the CPU.

Regression cases, named: test_band_set_and_cleared -- Engine::set_band_width(0) did not put the plan chosen at construction
back, so an engine whose band had been set and cleared stayed on the long-read path (describe: long_mode 1, ragged batching
silently off, other cells judged).  test_refused_alignment_call_reports_its_own_format -- a refused align_host /
align_cigar_host call left ran_result_format as the previous alignment call had set it ("cigar" after a refused rows call,
"rows" after a refused CIGAR call), where a new engine reports the refused call's own format; the sequences exposed it at
tiny, seed 2, step 30.  test_extension_alignment_reports_its_own_pointer_bytes -- an extension alignment on the register route
left align_ptr_bytes_per_pair as the last other alignment call had set it; comparing that key after every extension alignment
that ran exposed it."""
import functools

import pytest

import engine_sequences as es
from conftest import debug_switches

pytestmark = pytest.mark.gpu

CASES = [(world, scoring, seed) for world in ("tiny", "short", "long") for scoring in es.WORLDS[world]["scorings"]
         for seed in es.WORLDS[world]["seeds"]]


@functools.lru_cache(maxsize=None)
def _runner(world, scoring):
    return es.Runner(world, scoring)          # the pairs on the device and every reference, shared by the seeds


def _check_not_hidden(world, scoring, stats):
    assert 3 * stats["refused"] <= stats["calls"], ("more than a third of the calls were refused", stats)
    for entry in es.ENTRY_POINTS:
        if entry in es.NEVER_SUCCEEDS.get((world, scoring), ()):
            assert stats["succeeded"][entry] == 0, (entry, "is refused by definition here, and ran")
        else:           # (align_extend_* in the long world and under the wide scoring too: the Band route runs them)
            assert stats["succeeded"][entry] >= 2, (entry, "succeeded fewer than twice", stats)
    # the Band route, from what ran_extend / ran_extend_align said after calls that ran and were verified: every extension entry
    # point at least twice in every sequence (test_engine_sequences holds the generator to as many calls that should)
    for entry, routes in stats["routes"].items():
        assert routes.get("band", 0) >= 2, (entry, "ran on the Band route fewer than twice", stats["routes"])


@pytest.mark.parametrize("world,scoring,seed", CASES, ids=lambda v: str(v))
def test_live_engine_is_a_new_engine(world, scoring, seed, monkeypatch):
    debug_switches(monkeypatch, ragged_min=8)          # before any engine exists: the length classes at these batch sizes
    stats = _runner(world, scoring).run(seed)
    _check_not_hidden(world, scoring, stats)


@pytest.mark.parametrize("world", ("tiny", "short"))
def test_refused_alignment_call_reports_its_own_format(world, monkeypatch):
    """Under band_alignments = 1 without band_nw the NW variant's alignments are refused: a refused host-pointer rows call right
    after a CIGAR call that ran, and the mirror, must describe() themselves as a new engine does (ran_result_format, and
    ran_align_fill "none")."""
    debug_switches(monkeypatch, ragged_min=8)
    call = {"kind": "call", "begin": 5, "n": 40, "threads": 2, "mask": 0, "extended": 1}
    steps = [{"kind": "set", "key": "band_width", "value": es.WORLDS[world]["bands"][0]},
             {"kind": "set", "key": "band_alignments", "value": 1},
             dict(call, entry="align_cigar_device", alg=es.SW), dict(call, entry="align_host", alg=es.NW),
             dict(call, entry="align_device", alg=es.SW), dict(call, entry="align_cigar_host", alg=es.NW),
             dict(call, entry="align_cigar_host", alg=es.SW), dict(call, entry="align_host", alg=es.NW, n=7),
             dict(call, entry="align_host", alg=es.SW), dict(call, entry="align_cigar_host", alg=es.NW, n=7)]
    for scoring in ("linear", "affine4"):
        stats = _runner(world, scoring).run(steps=steps)
        assert stats["calls"] == 8 and stats["refused"] == 4, stats
        assert all(stats["succeeded"][e] == 1 for e in ("align_cigar_device", "align_device", "align_cigar_host", "align_host")), stats


def test_band_set_and_cleared(monkeypatch):
    """The short world: a band is set, used and cleared, then every family that reads the plan is called -- and ragged batching
    must apply again, score_cells agree and a score_width = 16 judgement be a new engine's."""
    debug_switches(monkeypatch, ragged_min=8)
    call = {"kind": "call", "alg": es.SW, "begin": 3, "n": 130, "threads": 2, "mask": 75, "extended": 1}
    steps = [{"kind": "set", "key": "ragged_batching", "value": 2},
             {"kind": "set", "key": "band_width", "value": 16}, dict(call, entry="score_device"),
             {"kind": "set", "key": "band_width", "value": 0}]
    steps += [dict(call, entry=e) for e in ("score_device", "score_host", "align_device", "score_placed_device", "score_span_host",
                                            "score_subopt_device", "align_cigar_host")]
    steps += [{"kind": "set", "key": "score_width", "value": 16}, dict(call, entry="score_device", alg=es.NW), dict(call, entry="score_host", n=40)]
    for scoring in ("linear", "wide"):
        stats = _runner("short", scoring).run(steps=steps)
        assert stats["calls"] == 10


# ---- the state the newer entry points share: one hand-written sequence each ----
CALL = {"kind": "call", "alg": es.SW, "begin": 3, "n": 130, "threads": 2, "mask": 0, "extended": 1, "end_bonus": 5, "with_extend": 1}


def _set(key, value):
    return {"kind": "set", "key": key, "value": value}


def _counts(stats):
    return {e: k for e, k in stats["succeeded"].items() if k}


@pytest.mark.parametrize("world,scorings", [("short", ("linear", "affine4")), ("long", ("linear", "sym_affine"))])
def test_spanned_calls_share_one_child_engine(world, scorings, monkeypatch):
    """score_span_* and align_span_* re-key ONE child engine of the window's shape, whichever of them runs first creates it, and
    each copies its own set of keys: both score_width and placed_wide, only the CIGAR calls trace_checkpoints and
    pointer_scratch_cap_mb.  span -> span_cigar -> span with those keys flipped in between; in the long world the window's
    alignment takes the row strips, checkpointed under the key."""
    debug_switches(monkeypatch, ragged_min=8)
    steps = [dict(CALL, entry="score_span_device"),
             _set("trace_checkpoints", 1), _set("pointer_scratch_cap_mb", 2),
             dict(CALL, entry="align_span_device"), dict(CALL, entry="score_span_host", n=40), dict(CALL, entry="align_span_host", extended=0),
             _set("score_width", 32), _set("placed_wide", 1),
             dict(CALL, entry="score_span_device", n=7), dict(CALL, entry="align_span_device", begin=20),
             _set("score_width", 0),
             dict(CALL, entry="align_span_host", n=40), dict(CALL, entry="score_span_device", begin=11),
             _set("trace_checkpoints", 0),
             dict(CALL, entry="align_span_device", n=40, extended=0), dict(CALL, entry="score_span_host")]
    for scoring in scorings:
        stats = _runner(world, scoring).run(steps=steps)
        assert stats["calls"] == 10 and stats["refused"] == 0, stats
        assert _counts(stats) == {"score_span_device": 3, "score_span_host": 2, "align_span_device": 3, "align_span_host": 2}, stats


@pytest.mark.parametrize("world", ("short", "tiny"))
def test_cigar_rows_scratch_at_two_pitches(world, monkeypatch):
    """Extension alignments walk in the pointer scratch, the end cells and the rows of align_cigar_* -- at a row pitch of
    R + F + 1 where align_cigar_* has R + F; the buffers only grow.  A banded alignment sizes them first, then the two kinds of
    call alternate at batch sizes that shrink and grow again."""
    debug_switches(monkeypatch, ragged_min=8)
    always = es.END_BONUSES[-1]
    steps = [_set("band_width", es.WORLDS[world]["bands"][0]), _set("band_alignments", 1), dict(CALL, entry="align_cigar_device", n=40),
             _set("band_width", 0),
             dict(CALL, entry="align_cigar_device"), dict(CALL, entry="align_extend_device"), dict(CALL, entry="align_cigar_host", n=7),
             dict(CALL, entry="align_extend_host", end_bonus=-1), dict(CALL, entry="align_device", n=40),
             dict(CALL, entry="align_extend_device", n=1, begin=64, end_bonus=always), dict(CALL, entry="align_cigar_device", extended=0),
             dict(CALL, entry="align_extend_host", n=7, with_extend=0, extended=0), dict(CALL, entry="align_cigar_host", begin=30),
             dict(CALL, entry="align_extend_device", begin=30, end_bonus=always, with_extend=0)]
    for scoring in ("linear", "affine4"):
        stats = _runner(world, scoring).run(steps=steps)
        assert stats["calls"] == 11 and stats["refused"] == 0, stats
        assert _counts(stats) == {"align_cigar_device": 3, "align_cigar_host": 2, "align_device": 1, "align_extend_device": 3, "align_extend_host": 2}, stats


@pytest.mark.parametrize("world,scorings", [("short", ("wide",)), ("long", ("linear", "affine4"))])
def test_int32_sweeps_share_the_strip_scratch(world, scorings, monkeypatch):
    """extend_wide runs its int32 sweep on the boundary rows and end cells of the placed int32 sweep (include/valign_hip.h:
    "shared with it: calls of one engine that use it belong on one stream").  The two alternate on one engine and one stream at
    130, 7 and 130 pairs: 150 x 600 leaves int16 by itself, the long world's placed scores take int32 cells under
    score_width = 32.  Then each key is cleared, and the call it had opened is refused again."""
    debug_switches(monkeypatch, ragged_min=8)
    steps = [_set("placed_wide", 1), _set("extend_wide", 1)] + ([_set("score_width", 32)] if world == "long" else [])
    for n in (130, 7, 130):
        steps += [dict(CALL, entry="score_placed_device", n=n), dict(CALL, entry="score_extend_device", n=n)]
    steps += [dict(CALL, entry="score_placed_host", n=40), dict(CALL, entry="score_extend_host", n=40),
              _set("placed_wide", 0), dict(CALL, entry="score_placed_device"), dict(CALL, entry="score_extend_device", begin=9),
              _set("extend_wide", 0), dict(CALL, entry="score_extend_device", n=7)]
    for scoring in scorings:
        stats = _runner(world, scoring).run(steps=steps)
        assert stats["calls"] == 11 and stats["refused"] == 2, stats
        assert _counts(stats) == {"score_placed_device": 3, "score_placed_host": 1, "score_extend_device": 4, "score_extend_host": 1}, stats


@pytest.mark.parametrize("world", ("short", "tiny"))
def test_extend_wide_flips_around_a_refusal(world, monkeypatch):
    """extend_wide picks the route of an extension call and whether align_extend_* is refused at all: under extend_wide = 1 with
    score_width = 32 the scores run wide and the alignments are refused with a text of their own; score_width = 0 lets them
    run, extend_wide = 0 changes nothing for them, and score_width = 32 then refuses both with the scores' text.  After every
    call, refused ones included, ran_extend* / ran_extend_align* are a new engine's."""
    debug_switches(monkeypatch, ragged_min=8)
    steps = [_set("extend_wide", 1), _set("score_width", 32),
             dict(CALL, entry="score_extend_device"), dict(CALL, entry="align_extend_device"),
             dict(CALL, entry="score_extend_host", n=40), dict(CALL, entry="align_extend_host", n=40),
             _set("score_width", 0),
             dict(CALL, entry="align_extend_device"), dict(CALL, entry="score_extend_device", n=7), dict(CALL, entry="align_extend_host", n=7),
             _set("extend_wide", 0),
             dict(CALL, entry="align_extend_device", n=40, with_extend=0), dict(CALL, entry="score_extend_host"),
             _set("score_width", 32),
             dict(CALL, entry="score_extend_device", n=1), dict(CALL, entry="align_extend_device", n=1)]
    for scoring in ("linear", "sym_affine"):
        lines = []
        stats = _runner(world, scoring).run(steps=steps, log=lines.append)
        assert stats["calls"] == 11 and stats["refused"] == 4, stats
        assert _counts(stats) == {"score_extend_device": 2, "score_extend_host": 2, "align_extend_device": 2, "align_extend_host": 1}, stats
        refused = [line.partition(" -> refused ")[2] for line in lines if " -> refused " in line]
        assert len(refused) == 4 and all(text.startswith("extension alignments:") for text in refused[:2]), refused
        assert all("score_width = 32" in text and not text.startswith("extension alignments:") for text in refused[2:]), refused


# ---- the Band route of the two extension families (extend_band, extend_band_align) and the state it shares ----
ALWAYS = es.END_BONUSES[-1]
NO_BAND_TEXT = "extension scores are not built for band_width > 0"


def _band_routes(stats):
    return {e: routes.get("band", 0) for e, routes in stats["routes"].items() if routes.get("band", 0)}


@pytest.mark.parametrize("world,scorings", [("short", ("wide",)), ("long", ("linear", "affine4")), ("strips", ("linear", "affine4"))])
def test_band_route_shares_the_strip_scratch(world, scorings, monkeypatch):
    """The Band route's boundary rows and partial records lie in the strip scratch (Engine::d_placed_rows_ / d_placed_ends_) of the
    placed int32 sweep, of extend_wide and of the placed strip route, each with a record layout and sizes of its own.  With
    placed_wide = extend_wide = extend_band = extend_band_align = 1 one engine rotates, at 130, 7, 1 and 130 pairs (7 and 1 are
    odd: a wave is two pairs, the scratch is sized by pairs + 1): an unbanded placed call (150 x 600: the int32 sweep; the long
    world under score_width = 0: the strip route), an unbanded extension-score call (extend_wide's int32 sweep in both), then
    under a band banded extension scores and alignments through the device and the host entries, then no band again.  In the long
    world a spanned CIGAR call follows a banded extension alignment."""
    debug_switches(monkeypatch, ragged_min=8)
    band = es.WORLDS[world]["bands"][0]
    steps = [_set(key, 1) for key in ("placed_wide", "extend_wide", "extend_band", "extend_band_align")]
    for k, (n, begin) in enumerate(((130, 3), (7, 20), (1, 64), (130, 30))):
        call = dict(CALL, n=n, begin=begin)
        steps += [dict(call, entry="score_placed_device"), dict(call, entry="score_extend_device"),
                  _set("band_width", band),
                  dict(call, entry="score_extend_device"), dict(call, entry="align_extend_device", end_bonus=es.END_BONUSES[k], with_extend=k % 2),
                  dict(call, entry="score_extend_host"), dict(call, entry="align_extend_host", end_bonus=es.END_BONUSES[3 - k], with_extend=1 - k % 2),
                  _set("band_width", 0)]
        if world == "long" and k == 1:
            steps.append(dict(call, entry="align_span_device"))
    spans = 1 if world == "long" else 0
    for scoring in scorings:
        stats = _runner(world, scoring).run(steps=steps)
        assert stats["calls"] == 24 + spans and stats["refused"] == 0, stats
        want = {"score_placed_device": 4, "score_extend_device": 8, "score_extend_host": 4, "align_extend_device": 4, "align_extend_host": 4}
        assert _counts(stats) == (dict(want, align_span_device=1) if spans else want), stats
        assert _band_routes(stats) == {"score_extend_device": 4, "score_extend_host": 4, "align_extend_device": 4, "align_extend_host": 4}, stats
        if world != "strips":           # the unbanded extension scores between them ran on extend_wide's int32 sweep, on the same scratch
            assert stats["routes"]["score_extend_device"] == {"band": 4, "wide": 4}, stats


@pytest.mark.parametrize("world", ("short", "tiny", "strips"))
def test_band_route_shares_the_pointer_scratch(world, monkeypatch):
    """The Band route's pointer regions and end cells lie in the pointer scratch of every alignment fill (d_ptr_ / d_ends_), cut
    into chunks under pointer_scratch_cap_mb, and its walk writes the CIGAR rows scratch at a pitch of R + F + 1 where
    align_cigar_* has R + F.  Under a cap of 2 MB a banded Smith-Waterman alignment (band_alignments = 1) sizes the scratch first;
    then banded extension alignments at 130, 7 and 130 pairs alternate with unbanded CIGAR calls and unbanded extension alignments
    on the register route, with trace_checkpoints = 1 from partway on (not at 520 rows: more than one strip).  At 520 x 600 a pair
    of the band of 40 holds at least 87 KB of pointers (tests/test_gpu_extend_band_align.py::test_chunks pins 175 to 512 KB with
    affine gaps, linear gaps take half), so the 130-pair call cannot fit 2 MB: the live engine must report more than one chunk."""
    debug_switches(monkeypatch, ragged_min=8)
    band = es.WORLDS[world]["bands"][0]
    steps = [_set("pointer_scratch_cap_mb", 2), _set("band_width", band), _set("band_alignments", 1), dict(CALL, entry="align_cigar_device", n=40),
             _set("extend_band", 1), _set("extend_band_align", 1)]
    big = len(steps)
    steps += [dict(CALL, entry="align_extend_device"),
              _set("band_width", 0),
              dict(CALL, entry="align_cigar_device"), dict(CALL, entry="align_extend_host", end_bonus=-1),
              _set("band_width", band),
              dict(CALL, entry="align_extend_host", n=7, with_extend=0),
              _set("band_width", 0)]
    if world != "strips":
        steps.append(_set("trace_checkpoints", 1))
    steps += [dict(CALL, entry="align_cigar_host", n=7, extended=0), dict(CALL, entry="align_extend_device", n=40, end_bonus=ALWAYS),
              _set("band_width", band),
              dict(CALL, entry="align_extend_device", begin=30, end_bonus=ALWAYS),
              _set("band_width", 0),
              dict(CALL, entry="align_cigar_host", begin=30),
              _set("band_width", band),
              dict(CALL, entry="align_extend_host", begin=9, extended=0)]
    for scoring in ("linear", "affine4"):
        stats = _runner(world, scoring).run(steps=steps)
        assert stats["calls"] == 10 and stats["refused"] == 0, stats
        assert _counts(stats) == {"align_cigar_device": 2, "align_cigar_host": 2, "align_extend_device": 3, "align_extend_host": 3}, stats
        assert stats["routes"]["align_extend_device"] == {"band": 2, "rows": 1} and stats["routes"]["align_extend_host"] == {"band": 2, "rows": 1}, stats
        if world == "strips":
            assert stats["chunks"][big] > 1, ("the 130-pair banded call was not cut into chunks", stats["chunks"])


@pytest.mark.parametrize("world", ("short", "strips"))
def test_two_bands_on_one_engine(world, monkeypatch):
    """The pointer layout of a banded extension alignment (versalignlib_amd/csrc/extend_band_align_plan.h) and the windows of the
    banded sweep depend on w = band_width / 2: one engine runs banded extension scores and alignments under the world's first
    band, its second and the first again, at 130, 40 and 130 pairs, with all four end bonuses.  In the short world a spanned CIGAR
    call stands between two of the banded alignments (the band cleared around it)."""
    debug_switches(monkeypatch, ragged_min=8)
    bands = es.WORLDS[world]["bands"]
    steps = [_set("extend_band", 1), _set("extend_band_align", 1)]
    for k, (band, n) in enumerate(((bands[0], 130), (bands[1], 40), (bands[0], 130))):
        call = dict(CALL, n=n, begin=3 + 10 * k)
        steps += [_set("band_width", band),
                  dict(call, entry="align_extend_device", end_bonus=es.END_BONUSES[k]), dict(call, entry="score_extend_device"),
                  dict(call, entry="align_extend_host", end_bonus=es.END_BONUSES[3 - k], with_extend=k % 2)]
        if world == "short" and k == 0:
            steps += [_set("band_width", 0), dict(call, entry="align_span_device", n=40)]
    spans = 1 if world == "short" else 0
    for scoring in ("linear", "affine4"):
        stats = _runner(world, scoring).run(steps=steps)
        assert stats["calls"] == 9 + spans and stats["refused"] == 0, stats
        want = {"score_extend_device": 3, "align_extend_device": 3, "align_extend_host": 3}
        assert _counts(stats) == (dict(want, align_span_device=1) if spans else want), stats
        assert _band_routes(stats) == want, stats


@pytest.mark.parametrize("world", ("tiny", "short"))
def test_extend_band_keys_flip_around_refusals(world, monkeypatch):
    """The route of an extension call is picked by band_width, extend_band, extend_band_align and score_width together, and a
    refused call must fall back to "none" with the text a new engine gives (include/valign_hip.h).  Under a band: both keys off --
    both families refused with the scores' text; extend_band = 1 -- the scores run banded, the alignments are refused with a text
    of their own; extend_band_align = 1 -- both run; score_width = 16 -- both refused with a text that begins "extend_band:";
    score_width = 32 -- both run; extend_band = 0 with extend_band_align still 1 -- both refused with the scores' text again;
    band_width = 0 (and score_width = 0, which the register route needs) -- the register route.  After every call, refused ones
    included, ran_extend* / ran_extend_align* are a new engine's."""
    debug_switches(monkeypatch, ragged_min=8)
    steps = [_set("band_width", es.WORLDS[world]["bands"][1]),
             dict(CALL, entry="score_extend_device"), dict(CALL, entry="align_extend_device"),
             _set("extend_band", 1),
             dict(CALL, entry="score_extend_host"), dict(CALL, entry="align_extend_host"),
             _set("extend_band_align", 1),
             dict(CALL, entry="score_extend_device", n=40), dict(CALL, entry="align_extend_device"),
             _set("score_width", 16),
             dict(CALL, entry="score_extend_device"), dict(CALL, entry="align_extend_host", n=40),
             _set("score_width", 32),
             dict(CALL, entry="score_extend_host", n=7), dict(CALL, entry="align_extend_device", n=7, end_bonus=ALWAYS),
             _set("extend_band", 0),
             dict(CALL, entry="score_extend_device", n=1), dict(CALL, entry="align_extend_device", n=1),
             _set("band_width", 0), _set("score_width", 0),
             dict(CALL, entry="score_extend_device"), dict(CALL, entry="align_extend_host", with_extend=0)]
    for scoring in ("linear", "sym_affine"):
        lines = []
        stats = _runner(world, scoring).run(steps=steps, log=lines.append)
        assert stats["calls"] == 14 and stats["refused"] == 7, stats
        assert _counts(stats) == {"score_extend_device": 2, "score_extend_host": 2, "align_extend_device": 2, "align_extend_host": 1}, stats
        assert stats["routes"] == {"score_extend_device": {"band": 1, "rows": 1}, "score_extend_host": {"band": 2}, "align_extend_device": {"band": 2},
                                   "align_extend_host": {"rows": 1}}, stats
        refused = [line.partition(" -> refused ")[2].strip() for line in lines if " -> refused " in line]
        assert len(refused) == 7, refused
        assert refused[0] == refused[1] == refused[5] == refused[6] == NO_BAND_TEXT, refused
        assert refused[2].startswith("extension alignments: not built under a band"), refused
        assert refused[3].startswith("extend_band:") and refused[4].startswith("extend_band:") and "score_width = 16" in refused[3], refused


def test_extension_alignment_reports_its_own_pointer_bytes(monkeypatch):
    """Regression, named: an extension alignment on the register route left align_ptr_bytes_per_pair as the last OTHER alignment call
    had set it (describe: "the pointer-stream bytes a pair holds in the plan of the last alignment call"), so a live engine
    reported a CIGAR call's -- or a banded extension alignment's -- figure where a new engine reports the call's own.  A register
    extension alignment after an unbanded CIGAR call, after a banded extension alignment, and first of all."""
    debug_switches(monkeypatch, ragged_min=8)
    steps = [dict(CALL, entry="align_extend_device", n=40),
             dict(CALL, entry="align_cigar_device"), dict(CALL, entry="align_extend_device"),
             _set("extend_band", 1), _set("extend_band_align", 1), _set("band_width", 16),
             dict(CALL, entry="align_extend_host"),
             _set("band_width", 0),
             dict(CALL, entry="align_extend_host", n=7)]
    for scoring in ("linear", "affine4"):
        stats = _runner("short", scoring).run(steps=steps)
        assert stats["calls"] == 5 and stats["refused"] == 0, stats
        assert stats["routes"]["align_extend_device"] == {"rows": 2} and stats["routes"]["align_extend_host"] == {"band": 1, "rows": 1}, stats
