"""The lane map of the score kernels (versalignlib_amd/csrc/lane_map.h) on the CPU.  tests/lane_map_check.cpp includes the pure
header and is built with plain g++ -- no HIP, no GPU: the bijection, the previous lane, the leaders a DPP row shift zeroes, the
reduction distances and the halves of the wave, for the contiguous and the interleaved map.  Then a numpy restatement of the lane
hand-over of the tilted sweep's step (dp_kernels.hip.h: group_prev_or / row_prev_or) on 64 lanes under both maps: what lane l
of group grp reads as the row above its row 0 is the same value under either, F's source and the moving border alike."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "lane_map_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")
WAVE, ROW = 64, 16


def test_lane_map_check(tmp_path):
    exe = str(tmp_path / "lane_map_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "lane map ok" in res.stdout, res.stdout[-3000:]


def test_the_kernel_takes_its_lanes_from_the_map_and_the_check_is_sanitized():
    text = open(os.path.join(CSRC, "dp_kernels.hip.h")).read()
    assert '#include "lane_map.h"' in text and text.count("LaneMap<G, score_lane_stride(G, K)>") == 2      # the set-up and the kernel
    assert "lmap::grp(lane)" in text and "lmap::l(lane)" in text and "lmap::reduce_distance(i)" in text
    assert "row_prev_or<lmap::kStride>" in text and "row_prev_or_zero<lmap::kStride>" in text
    assert "#include <hip" not in open(os.path.join(CSRC, "lane_map.h")).read()                           # a pure header
    assert "lane_map_check.cpp" in open(os.path.join(ROOT, "tools", "sanitize.sh")).read()


# ---- the maps, restated ----
def lane_of(G, S, grp, l):
    return (grp // S) * ROW + l * S + grp % S if S > 1 else grp * G + l


def grp_l(G, S, lane):
    return ((lane // ROW) * S + lane % S, (lane % ROW) // S) if S > 1 else (lane // G, lane % G)


def wave_shr1(v):
    """v_mov_b32_dpp wave_shr:1 onto a zero: lane - 1's value, 0 in lane 0"""
    return np.concatenate(([0], v[:-1]))


def row_shr(v, n):
    """v_mov_b32_dpp row_shr:n bound_ctrl: lane - n's value inside the 16-lane row, 0 where the source lies before the row"""
    out = np.zeros_like(v)
    for lane in range(WAVE):
        if lane % ROW >= n:
            out[lane] = v[lane - n]
    return out


def hand_over(G, S, value, border):
    """The row above row 0 of every lane -> {(grp, l): what the lane reads}.  value(grp, l): the last row of lane l of group grp
    (never 0); border(grp): what the group's first lane reads instead."""
    v = np.zeros(WAVE, dtype=np.int64)
    lead = np.zeros(WAVE, dtype=np.int64)            # lead_border: the border in the leaders, 0 in every other lane
    lmask = np.zeros(WAVE, dtype=np.int64)           # 0 in the leaders, all ones elsewhere
    for lane in range(WAVE):
        grp, l = grp_l(G, S, lane)
        v[lane] = value(grp, l)
        lead[lane] = border(grp) if l == 0 else 0
        lmask[lane] = 0 if l == 0 else -1
    if S > 1:
        got = row_shr(v, S) | lead                   # row_prev_or: one v_or_b32 with a DPP operand
    else:
        got = (wave_shr1(v) & lmask) | lead          # group_prev_or<8>: the shift, the mask, the border
    return {grp_l(G, S, lane): int(got[lane]) for lane in range(WAVE)}


@pytest.mark.parametrize("G", (8, 4))
def test_the_hand_over_reads_the_same_row_under_both_maps(G):
    S = ROW // G
    for lane in range(WAVE):
        assert lane_of(G, S, *grp_l(G, S, lane)) == lane and lane_of(G, 1, *grp_l(G, 1, lane)) == lane
    value = lambda grp, l: 0x10000 + 0x100 * grp + l + 1        # distinct and non-zero: a neighbour group's value is seen
    for border in (lambda grp: 0, lambda grp: 0x4000000 + grp):  # F's source (the shift's zero) and the moving border
        contiguous, interleaved = hand_over(G, 1, value, border), hand_over(G, S, value, border)
        assert sorted(contiguous) == sorted(interleaved) == [(grp, l) for grp in range(WAVE // G) for l in range(G)]
        for (grp, l), got in interleaved.items():
            want = border(grp) if l == 0 else value(grp, l - 1)
            assert got == want == contiguous[(grp, l)], (G, grp, l, got, want, contiguous[(grp, l)])


def test_the_shift_alone_is_not_the_hand_over_for_contiguous_groups_of_8():
    """what the mask is for: without it lane 8 of a DPP row reads the last lane of the neighbour group"""
    v = np.arange(1, WAVE + 1, dtype=np.int64)
    leaders = [lane for lane in range(WAVE) if lane % 8 == 0]
    assert [int(wave_shr1(v)[lane]) for lane in leaders] == [0] + [lane for lane in leaders[1:]]
    assert [lane for lane in range(WAVE) if row_shr(v, 2)[lane] == 0] == [lane for lane in range(WAVE) if grp_l(8, 2, lane)[1] == 0]
