"""The plan of the row-strip alignment path (versalignlib_amd/csrc/strip_plan.h) as the engine runs it: at 1025 x 200 -- the
shortest read that takes strips unforced, two strips at 12 rows per lane -- every strip mode returns the oracle's alignments,
ran_align_fill names the route, and the bytes per pair describe() reports are those of the rows per lane the rule predicts
(which is what pins the geometry choice on the device: the full-pointer figure separates 16 rows per lane from 12 and 8, whose
strips x rows agree at this read length; the checkpointed figures, one region and S - 1 row sets, separate 12 from 8).  Three pairs:
half of the last wave is empty."""
import functools

import numpy as np
import pytest

from oracle import cpu_ref
from versalignlib_amd import hipkernel, host, synth
import band_align_ref as bar
import band_nw_ref as bnr

pytestmark = pytest.mark.gpu

R, F, N = 1025, 200, 3
BAND = 64
AFFINE = (-5, -1, -4, -2)
WIDE_SCALE = 150          # scores x 150: cells leave int16 (cell_rules.h: strip_wide), as tests/test_gpu_long.py
WALK_STATE_BYTES = 24

# name -> alg, scoring (match, mismatch, gap_read, gap_ref[, affine]), engine keys, route, the rows per lane compiled for the mode
CASES = {
    "linear-sw": (host.SW, (2, -1, -3, -2), {}, "strip", (16, 12, 8)),
    "linear-nw": (host.NW, (2, -1, -3, -2), {}, "strip", (16, 12, 8)),
    "affine-sw": (host.SW, (2, -1, -3, -3) + AFFINE, {}, "strip", (16, 12, 8)),
    "affine-nw": (host.NW, (2, -1, -3, -3) + AFFINE, {}, "strip", (16, 12, 8)),
    "sse-sw": (host.SW, (2, -1, -3, -2), dict(traceback_policy=1), "strip", (16, 12, 8)),
    "sse-nw": (host.NW, (2, -1, -3, -2), dict(traceback_policy=1), "strip", (16, 12, 8)),
    "ckpt-sw": (host.SW, (2, -1, -3, -2), dict(trace_checkpoints=1), "strip_ckpt", (16, 12, 8)),
    "ckpt-affine-nw": (host.NW, (2, -1, -3, -3) + AFFINE, dict(trace_checkpoints=1), "strip_ckpt", (16, 12, 8)),
    "band-sw": (host.SW, (2, -1, -3, -2), dict(band_width=BAND, band_alignments=1), "strip_band", (16, 8)),
    "band-affine-sw": (host.SW, (2, -1, -3, -3) + AFFINE, dict(band_width=BAND, band_alignments=1), "strip_band", (16, 8)),
    "band-nw": (host.NW, (2, -1, -3, -2), dict(band_width=BAND, band_alignments=1, band_nw=1), "strip_band", (16, 8)),
    "int32-sw": (host.SW, tuple(WIDE_SCALE * v for v in (2, -1, -3, -4)), {}, "strip_wide", (8,)),
    "int32-nw": (host.NW, tuple(WIDE_SCALE * v for v in (2, -1, -3, -4)), {}, "strip_wide", (16, 12, 8)),
}


@functools.lru_cache(maxsize=None)
def _pairs():
    return synth.make_pairs(N, R, F, seed=1025, sub_rate=0.08, indel_rate=0.02, n_run_frac=0.15, short_frac=0.25, lowercase_frac=0.05,
                            junk_frac=0.03)


def rows_per_lane(ks):
    """The rule of strip_plan.h restated: padded rows x {1.0, 1.115, 1.147}, the first of 16, 12, 8 wins a tie."""
    cost = {k: -(-R // (64 * k)) * 64 * k * {16: 1.0, 12: 1.115, 8: 1.147}[k] for k in ks}
    return min(sorted(ks, reverse=True), key=lambda k: cost[k])


def bytes_per_pair(K, affine, wide, ckpt, band):
    """-> align_ptr_bytes_per_pair, align_ckpt_bytes_per_pair of the plan at K rows per lane; band: None or (width, block_rows, col_align)."""
    rows = 64 * K
    S = max(1, -(-R // rows))
    pad = S * rows - R
    max_cols = F
    if band:
        max_cols = 0
        for s in range(S):
            lo, _ = bar.row_window(max(0, s * rows - pad), R, F, *band)
            _, hi = bar.row_window((s + 1) * rows - pad - 1, R, F, *band)
            max_cols = max(max_cols, hi - lo + 1)
    blocks8 = (max_cols + 70) // 8
    row_dwords = ((F + 71) // 64 + 2) * 64
    strip_words = blocks8 * 64 * K * (2 if affine else 1)
    row_sets = (2 if affine else 1) * (2 if wide else 1)
    if ckpt:
        return 4 * strip_words // 2, ((S - 1) * row_sets * row_dwords * 4 + 2 * WALK_STATE_BYTES) // 2
    return 4 * strip_words * S // 2, 0


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_strip_mode_on_the_planned_geometry(case):
    alg, scores, keys, route, ks = CASES[case]
    affine, wide, ckpt = len(scores) > 4, route == "strip_wide", route == "strip_ckpt"
    reads, refs = _pairs()
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*scores))
    for key, value in keys.items():
        getattr(eng, "set_" + key)(value)
    got = eng.align_host(alg, reads, refs, threads=2)
    d = eng.describe(alg, N)
    eng.close()
    sc = cpu_ref.Scoring.make(*scores)
    band = None
    if "band_width" in keys:
        band = (BAND, d["band_block_rows"], d["band_col_align"])
        exp = (bar.align_banded_sw if alg == host.SW else bnr.align_banded_nw)(reads, refs, BAND, sc, band[1], band[2], affine=affine)
    else:
        exp = cpu_ref.align(alg, reads, refs, sc, threads=4, affine=affine, wide=wide, **(dict(policy="sse") if "traceback_policy" in keys else {}))
    assert d["ran_align_fill"] == route, d
    K = rows_per_lane(ks)
    assert K == (8 if (band or case == "int32-sw") else 12)        # (the CPU check pins the same: two strips of 768, three of 512)
    print(case, "K", K, "ptr", d["align_ptr_bytes_per_pair"], "ckpt", d["align_ckpt_bytes_per_pair"], "expected", bytes_per_pair(K, affine, wide, ckpt, band))
    assert (d["align_ptr_bytes_per_pair"], d["align_ckpt_bytes_per_pair"]) == bytes_per_pair(K, affine, wide, ckpt, band), d
    assert np.array_equal(got[1], exp[1]), (case, "idx", got[1], exp[1])
    bad = np.nonzero((got[0] != exp[0]).any(axis=(1, 2)))[0]
    assert bad.size == 0, (case, "rows", bad)
