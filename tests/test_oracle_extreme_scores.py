"""The int32 oracle pinned by exhaustive enumeration at scorings far outside int16.

Beyond the int16 range of the DP cells the GPU suite judges the kernels with the oracle's own int32 restatement
(cpu_ref.score / align with wide=True): the reference wraps there, so nothing of the reference pins those numbers.
Here tiny pairs (at most 6 x 6) are judged by tests/enumerate_alignments.py, which walks every alignment and shares
no code with the oracle: scores (saturated to the ABI's short, as the oracle documents), the end cell of each
alignment and the score its rows re-score to.  Match up to 32767; mismatch, gaps, openings and extensions down to
-32768; extension equal to the opening and cheaper than it; both modes."""
import numpy as np
import pytest

import enumerate_alignments as en
from oracle import cpu_ref

# (match, mismatch, open_read, ext_read, open_ref, ext_ref); linear rows have open == ext in each direction
LINEAR = [
    (32767, -32768, -32768, -32768, -32768, -32768),
    (12000, -1, -1, -1, -1, -1),
    (1, -32768, -1, -1, -32768, -32768),
    (30000, -30000, -20000, -20000, -5, -5),
    (32767, 0, 0, 0, 0, 0),
    (9, -32768, -30000, -30000, -20000, -20000),
]
AFFINE = [
    (32767, -32768, -32768, -32768, -32768, -32768),        # extension == opening
    (20000, -20000, -32768, -1, -32768, -1),                # extension far cheaper than opening
    (9000, -4000, -30000, -100, -2, -2),
    (32767, -1, -5, -5, -32768, -32767),
    (3, -32768, -32767, -1, -32767, -1),
    (16384, -16384, -16385, -16384, -16384, -1),
]


def _pairs():
    """Tiny pairs built to reach the extremes: identical (the SW maximum min(R, F) * match in the last row),
    all-mismatch (the NW lower bounds), one long insertion / deletion, a repeat of the read in the reference
    (tied maxima), N runs, a junk byte and NUL-padded short sequences."""
    raw = [
        (b"ACG", b"ACG"), (b"ACGTAC", b"ACGTAC"), (b"AAAAAA", b"CCCCCC"), (b"ACGT", b"TGCA"),
        (b"ACGTTG", b"AC"), (b"AC", b"ACGTTG"), (b"ACTG", b"ACTGACTG"[:6]), (b"GAGA", b"GAGAGA"),
        (b"ANNC", b"AGTC"), (b"AC\xffG", b"ACTG"), (b"ACG\0\0\0", b"ACGTA\0"), (b"T", b"TTTTTT"),
        (b"CCCCC", b"C"), (b"acgt", b"ACGT"), (b"ATATAT", b"TATATA"), (b"GGCC", b"GGAACC"),
    ]
    return raw


def _arrays(read, ref):
    return np.frombuffer(read, np.uint8)[None, :].copy(), np.frombuffer(ref, np.uint8)[None, :].copy()


def _oracle_scoring(sc):
    return cpu_ref.Scoring.make(sc[0], sc[1], sc[2], sc[4], sc[2], sc[3], sc[4], sc[5])


def _sat(v):
    return max(-32768, min(32767, v))


def _sw_end(cells, R, F):
    """first row-major cell holding the maximum (the reference's strict '>' scan)"""
    best, end = 0, None
    for i in range(R + 1):
        for j in range(F + 1):
            if cells.get((i, j), 0) > best:
                best, end = cells[(i, j)], (i, j)
    return best, end


@pytest.mark.parametrize("affine", [False, True], ids=["linear", "affine"])
@pytest.mark.parametrize("k", range(6))
def test_int32_oracle_equals_enumeration_far_outside_int16(affine, k):
    sc = (AFFINE if affine else LINEAR)[k]
    osc = _oracle_scoring(sc)
    policies = ["default"] if affine else ["default", "sse"]
    outside = False
    for read, ref in _pairs():
        reads, refs = _arrays(read, ref)
        R, F = len(read), len(ref)
        AL = R + F
        # scores: the enumerated optimum, saturated to a short
        best, end = _sw_end(en.sw_cells(reads[0], refs[0], sc), R, F)
        sw = best
        nw = en.nw_variant_score(reads[0], refs[0], sc)
        assert cpu_ref.score(0, reads, refs, osc, affine=affine, wide=True)[0] == _sat(sw), (read, ref, sc, "SW")
        assert cpu_ref.score(1, reads, refs, osc, affine=affine, wide=True)[0] == _sat(nw), (read, ref, sc, "NW")
        cells = en.nw_variant_align_cells(reads[0], refs[0], sc)
        outside = outside or sw > 32767 or min(cells.values()) < -32768
        # (the SSE tie-breaks take no diagonal step on a base that is not ACGT, SURVEY.md F3: judged on clean pairs only)
        for policy in (policies if set(read + ref) <= set(b"ACGT") else ["default"]):
            kw = dict(affine=True) if affine else dict(policy=policy)
            # SW alignment: rows that re-score to the optimum and (default tie-breaks) end in the first row-major cell
            # holding it
            rows, idx = cpu_ref.align(0, reads, refs, osc, wide=True, **kw)
            s = int(idx[0, 0])
            a, b = bytes(rows[0, 0, s:AL - 1]), bytes(rows[0, 1, s:AL - 1])
            if sw > 0:
                assert en.rescore_rows(a, b, sc) == sw, (read, ref, sc, policy, a, b)
                if policy == "default":
                    ei, ej = end
                    ra, rb = en.ungapped(a), en.ungapped(b)
                    assert bytes(read[ei - len(ra):ei]) == ra and bytes(ref[ej - len(rb):ej]) == rb, (read, ref, sc, a, b, end)
            if policy != "default":
                continue
            # NW alignment: the reference's end cell from the enumerated cells; the rows re-score to that cell's value
            rows, idx = cpu_ref.align(1, reads, refs, osc, wide=True, **kw)
            ei, ej = en.nw_variant_end_cell(reads[0], refs[0], cells)
            s = int(idx[0, 0])
            a, b = bytes(rows[0, 0, s:AL - 1]), bytes(rows[0, 1, s:AL - 1])
            assert en.ungapped(a) == bytes(read[:ei + 1]), (read, ref, sc, a, b)
            rb = en.ungapped(b)
            assert rb == bytes(ref[ej + 1 - len(rb):ej + 1]), (read, ref, sc, a, b)
            assert en.rescore_rows(a, b, sc) == cells[(ei + 1, ej + 1)], (read, ref, sc, a, b)
    assert outside, "no pair leaves the int16 range under %r" % (sc,)
