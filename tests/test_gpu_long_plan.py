"""The route of a long-read score call (versalignlib_amd/csrc/long_plan.h) as the engine runs it: one case per route at the
smallest shape that reaches it -- the scores equal the oracle's, ran_score_cells names the cell format the route predicts and
long_strip_rows / band_block_rows the geometry.  Nine pairs: the last wave (eight pairs at 16 x 10, two at 64 x 8) and the chain's
last quad are part empty.  tests/long_plan_check.cpp pins on the CPU which chain variant each banded shape takes: 528 x 528 the
unit-delay kernel, 513 x 513 and 513 x 300 the delay ring (two turns of the cycle each), and that 2 x 3853 at band 64 has no
chain plan (a reference ring beyond 2048 columns)."""
import functools

import numpy as np
import pytest

from oracle import cpu_ref
from versalignlib_amd import hipkernel, host, synth
from conftest import debug_switches
import band_nw_ref as bnr

pytestmark = pytest.mark.gpu

N = 9
AFFINE = (-5, -1, -5, -1)
WIDE = tuple(150 * v for v in (2, -1, -3, -4))       # scores x 150: cells leave int16, as tests/test_gpu_strip_plan.py
SCORINGS = {"sym": (2, -1, -3, -3), "two-gaps": (2, -1, -2, -4), "affine": (2, -1, -3, -3) + AFFINE}

# name -> R, F, alg, scoring, band_width, band_nw, debug switches, expected ran_score_cells, long_strip_rows, band_block_rows (None: unbanded)
CASES = {}
for _R, _rows in ((160, 160), (161, 160)):            # one strip (no boundary rows) / two 160-row strips
    CASES["%d-sw-sym" % _R] = (_R, 200, host.SW, SCORINGS["sym"], 0, 0, dict(force_long=1), "f16", _rows, None)
    CASES["%d-sw-two-gaps" % _R] = (_R, 200, host.SW, SCORINGS["two-gaps"], 0, 0, dict(force_long=1), "int16", _rows, None)
    CASES["%d-sw-affine" % _R] = (_R, 200, host.SW, SCORINGS["affine"], 0, 0, dict(force_long=1), "int16", _rows, None)
    CASES["%d-nw" % _R] = (_R, 200, host.NW, SCORINGS["sym"], 0, 0, dict(force_long=1), "int16", _rows, None)
for _alg, _a in ((host.SW, "sw"), (host.NW, "nw")):   # three 512-row strips
    CASES["1025-%s-linear" % _a] = (1025, 200, _alg, SCORINGS["sym"], 0, 0, dict(force_long=1), "int16", 512, None)
    CASES["1025-%s-affine" % _a] = (1025, 200, _alg, SCORINGS["affine"], 0, 0, dict(force_long=1), "int16", 512, None)
CASES["1025-short-strips"] = (1025, 200, host.SW, SCORINGS["sym"], 0, 0, dict(force_long=1, short_strips=1), "f16", 160, None)
CASES["161-int32"] = (161, 200, host.SW, WIDE, 0, 0, {}, "int32", 160, None)
CASES["1025-int32"] = (1025, 200, host.NW, WIDE, 0, 0, {}, "int32", 512, None)
for _R, _F in ((528, 528), (513, 513), (513, 300)):   # the chain: unit delay / the delay ring (twice); the same shapes on the banded strips
    for _name, _alg, _sc, _nw in (("sw-linear", host.SW, "sym", 0), ("sw-affine", host.SW, "affine", 0), ("nw-linear", host.NW, "sym", 1)):
        CASES["chain-%dx%d-%s" % (_R, _F, _name)] = (_R, _F, _alg, SCORINGS[_sc], 32, _nw, {}, "int32", None, 16)
        CASES["band-strips-%dx%d-%s" % (_R, _F, _name)] = (_R, _F, _alg, SCORINGS[_sc], 32, _nw, dict(no_band_chain=1), "int32" if _nw else "int16", 160, 160)
CASES["fallback-2x3853"] = (2, 3853, host.SW, SCORINGS["sym"], 64, 0, {}, "int16", 160, 160)


@functools.lru_cache(maxsize=None)
def _pairs(R, F):
    reads, refs = synth.make_pairs(N, R, F, seed=R * 7 + F, sub_rate=0.08, indel_rate=0.02 if R > 8 else 0.0, n_run_frac=0.15, short_frac=0.25,
                                   lowercase_frac=0.05, junk_frac=0.03)
    reads.setflags(write=False)
    refs.setflags(write=False)
    return reads, refs


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_long_route_on_the_planned_kernel(monkeypatch, case):
    R, F, alg, scores, band, band_nw, switches, cells, strip_rows, block_rows = CASES[case]
    affine = len(scores) > 4
    reads, refs = _pairs(R, F)
    debug_switches(monkeypatch, **switches)
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*scores))
    eng.set_band_width(band)
    eng.set_band_nw(band_nw)
    got = eng.score_host(alg, reads, refs, threads=2)
    d = eng.describe(alg, N)
    eng.close()
    sc = cpu_ref.Scoring.make(*scores)
    if not band:
        exp = cpu_ref.score(alg, reads, refs, sc, threads=4, affine=affine, wide=cells == "int32")
    elif alg == host.SW:
        exp = cpu_ref.score_banded_sw(reads, refs, band, sc, threads=4, block_rows=d["band_block_rows"], col_align=d["band_col_align"], affine=affine)
    else:
        exp = np.minimum(bnr.score_banded_nw(reads, refs, band, sc, d["band_block_rows"], d["band_col_align"], affine=affine), 32767).astype(np.int16)
    print(case, "cells", d["ran_score_cells"], "predicted", d["score_cells"], "strip rows", d["long_strip_rows"], "band block", d["band_block_rows"], d["band_col_align"])
    assert d["ran_score_cells"] == cells and d["score_cells"] == cells, d
    if strip_rows is not None:
        assert d["long_strip_rows"] == strip_rows, d
    if block_rows is not None:
        assert (d["band_block_rows"], d["band_col_align"]) == ((16, 1) if block_rows == 16 else (160, 4)), d
    assert np.array_equal(got, exp), (case, got, exp)
