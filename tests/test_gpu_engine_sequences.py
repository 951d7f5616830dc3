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
    extend_align_ref;
  * a NEW engine of the same shape and scoring, configured to the current state, that makes the same call on the same data:
    the same result or the same refusal with the same text, and the same describe() keys (engine_sequences.compared);
  * its own sentinel, where a device-resident call was refused.
A sequence must not hide behind refusals: at most a third of its calls end refused and every entry point succeeds at least
twice -- but for the suboptimal scores and the extension alignments where include/valign_hip.h refuses them whatever the keys
say (engine_sequences.NEVER_SUCCEEDS: reads of more than 1 024 rows; a scoring whose cells leave int16).

Four hand-written sequences, one per piece of state that the newer entry points share with the older ones and with each other:
test_spanned_calls_share_one_child_engine, test_cigar_rows_scratch_at_two_pitches, test_int32_sweeps_share_the_strip_scratch,
test_extend_wide_flips_around_a_refusal.

Regression cases, named: test_band_set_and_cleared -- Engine::set_band_width(0) did not put the plan chosen at construction
back, so an engine whose band had been set and cleared stayed on the long-read path (describe: long_mode 1, ragged batching
silently off, other cells judged).  test_refused_alignment_call_reports_its_own_format -- a refused align_host /
align_cigar_host call left ran_result_format as the previous alignment call had set it ("cigar" after a refused rows call,
"rows" after a refused CIGAR call), where a new engine reports the refused call's own format; the sequences exposed it at
tiny, seed 2, step 30."""
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
        else:
            assert stats["succeeded"][entry] >= 2, (entry, "succeeded fewer than twice", stats)


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
