// extend_band_align_plan.h -- the pointer layout of banded extension alignments (key extend_band_align; include/valign_hip.h has the
// definition): where the banded int32 extension sweep that also streams back pointers (align_extend_band_fill_kernel) puts the
// 2-bit code of a present cell, and where the walk (extend_band_walk_kernel) finds it.  Integers in, integers out; no HIP: one
// statement for the fill, the walk, the engine and the CPU check (tests/extend_band_align_plan_check.cpp compares every function
// with a direct enumeration).  The band, its strips and their step windows are extend_band_plan.h's.
//
// Layout: [pair-of-pairs][strip][block of 8 steps counted from the strip's t_begin][lane][W dwords], W = 8 with linear gaps (one
// dword per row of the lane) and 16 with affine gaps (8 dwords of H codes, then 8 dwords of gap codes).  Pair A of the wave sits in
// the low half of a dword, pair B in the high half; within a half step t's code lies at bits 2 * (7 - (t & 7)) -- t_begin is a
// multiple of 64, so the position depends on the step alone.  A wave's block is 2 / 4 KB of contiguous dwords.
// The regions are sized for the ENGINE's reference length F: a wave whose larger trimmed reference length is below it sweeps a
// window that ends earlier (t_end shrinks, t_begin does not move) and writes the first blocks of its region only; a strip whose
// window is empty holds no block at all.
#pragma once

#include "extend_band_plan.h"

namespace valign {

constexpr int kExtendBandAlignBlockSteps = 8;           // steps per pointer block: 2 bits x 8 = one half of a dword

// dwords per lane and block
__host__ __device__ inline int extend_band_align_lane_dwords(bool affine) { return (affine ? 2 : 1) * kExtendBandBlockRows; }

// strips of a read of R rows (at least one: strip 0 always runs)
__host__ __device__ inline int extend_band_align_strips(int R) {
    const int s = (R + kExtendBandStripRows - 1) / kExtendBandStripRows;
    return s > 0 ? s : 1;
}

// 8-step blocks of strip `strip`: ceil((t_end - t_begin) / 8) of its window, 0 for an empty strip
__host__ __device__ inline int extend_band_align_strip_blocks(int strip, int F, int w) {
    const ExtendBandStrip s = extend_band_strip(strip, F, w);
    if (s.empty) return 0;
    return (s.t_end - s.t_begin + kExtendBandAlignBlockSteps - 1) / kExtendBandAlignBlockSteps;
}

// blocks of the strips before `strip` (strip = the number of strips: all of them)
__host__ __device__ inline long long extend_band_align_blocks_before(int strip, int F, int w) {
    long long blocks = 0;
    for (int s = 0; s < strip; ++s) blocks += extend_band_align_strip_blocks(s, F, w);
    return blocks;
}

// dword offset of strip `strip` in a pair-of-pairs' region; with strip = the number of strips: the dwords of the region
__host__ __device__ inline long long extend_band_align_strip_base(int strip, int F, int w, bool affine) {
    return extend_band_align_blocks_before(strip, F, w) * 64 * extend_band_align_lane_dwords(affine);
}
__host__ __device__ inline long long extend_band_align_pp_dwords(int R, int F, int w, bool affine) {
    return extend_band_align_strip_base(extend_band_align_strips(R), F, w, affine);
}

// dword, from the strip's base, of word x of lane `lane` in block `block`
__host__ __device__ inline long long extend_band_align_word(int block, int lane, int x, bool affine) {
    return ((long long)block * 64 + lane) * extend_band_align_lane_dwords(affine) + x;
}
// bit position of step t's code in the dword of pair `half` (0: A, 1: B)
__host__ __device__ inline int extend_band_align_shift(int t, int half) { return 16 * half + 2 * (kExtendBandAlignBlockSteps - 1 - (t & (kExtendBandAlignBlockSteps - 1))); }

// Where the code of the present interior cell (i, j), 0 <= i, 0 <= j, of pair `half` lies: the dword from the pair-of-pairs'
// first, and the shift of its two bits.  gap_word: the gap codes of affine gaps (the H codes otherwise).
struct ExtendBandAlignSlot {
    long long dword;
    int shift;
};
__host__ __device__ inline ExtendBandAlignSlot extend_band_align_slot(int i, int j, int half, bool gap_word, int F, int w, bool affine) {
    const int strip = i / kExtendBandStripRows, in_strip = i - strip * kExtendBandStripRows;
    const int lane = in_strip / kExtendBandBlockRows, q = in_strip - lane * kExtendBandBlockRows;
    const int t = j + lane;                                                    // lane l sweeps column t - l at step t
    const int block = (t - extend_band_strip(strip, F, w).t_begin) / kExtendBandAlignBlockSteps;
    ExtendBandAlignSlot s;
    s.dword = extend_band_align_strip_base(strip, F, w, affine) + extend_band_align_word(block, lane, q + (gap_word ? kExtendBandBlockRows : 0), affine);
    s.shift = extend_band_align_shift(t, half);
    return s;
}

}  // namespace valign
