"""One engine through a whole sequence of key changes and calls (tests/engine_sequences.py), against the references and against
new engines.

Per (world, scoring, seed) ONE engine runs sequence(world, seed): device-resident calls go on one non-default stream into
preallocated, sentinel-filled outputs, back to back; the stream is waited for only before a host-pointer step and at the end
(the contract is one stream per engine; describe() is host-side state and is read right after every call).  Every call step is
held against
  * the reference of the operation its state selects, bit for bit -- the authority: oracle/cpu_ref for unbanded scores and
    alignments (the cell width of an alignment read from ran_align_fill, never "either"), cpu_ref.score_banded_sw /
    band_align_ref / band_nw_ref under a band on the block shape describe() reports, cigar_ref, placed_ref / placed_band_ref,
    span_ref, subopt_ref;
  * a NEW engine of the same shape and scoring, configured to the current state, that makes the same call on the same data:
    the same result or the same refusal with the same text, and the same describe() keys (engine_sequences.compared);
  * its own sentinel, where a device-resident call was refused.
A sequence must not hide behind refusals: at most a third of its calls end refused and every entry point succeeds at least
twice -- but for the suboptimal scores where include/valign_hip.h refuses them whatever the keys say
(engine_sequences.NEVER_SUCCEEDS: reads of more than 1 024 rows; a scoring whose cells leave int16).

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
