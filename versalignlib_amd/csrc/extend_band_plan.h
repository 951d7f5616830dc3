// extend_band_plan.h -- the band of banded extension scores (key extend_band; include/valign_hip.h has the definition): which
// cells are present, what a 512-row strip of the int32 extension sweep (extend_wide_kernels.hip.h) sweeps of it, and when the
// read end is unreached.  Integers in, integers out; no HIP: one definition for the engine, the kernel and the CPU check
// (tests/extend_band_rules_check.cpp compares every function with a direct enumeration).
//
// The band lies on the ANCHOR's diagonal i = j, not on the scaled diagonal i * F / R of the Smith-Waterman bands (band_window.h).
// Rows are taken in blocks of B = 8 consecutive read positions counted from row 0 -- one lane's rows on the sweep, so that a lane
// is wholly inside or wholly outside its window at any step.  With w = band_width / 2:
//   cell (i, j), 0 <= i, -1 <= j:  present iff 8 * (i / 8) - w <= j <= 8 * (i / 8) + 7 + w   (the border column is j = -1)
//   cell (-1, j):                  present iff j + 1 <= w                                    ((-1, -1) always)
#pragma once

#include "../../include/valign_hip.h"

#ifndef __HIPCC__       // plain g++ (the CPU check): the functions below are host functions
#define __host__
#define __device__
#endif

namespace valign {

constexpr int kExtendBandBlockRows = VALIGN_HIP_EXTEND_BAND_BLOCK_ROWS;     // B: the rows of one lane of the sweep
constexpr int kExtendBandStripRows = 64 * kExtendBandBlockRows;             // a strip of the sweep: 64 lanes
constexpr int kExtendBandColAlign = 64;         // the sweep's reference ring and boundary rows move in blocks of 64 columns

// w of a call.  A band with w >= max(R, F) holds every cell (the unbanded limit), so w is capped there: row + 7 + w stays far
// inside int for every shape the engine takes.
__host__ __device__ inline int extend_band_half(int band_width, int R, int F) {
    const int w = band_width / 2, cap = R > F ? R : F;
    return w < cap ? w : cap;
}

// The window [lo, hi] of the block that holds read row `row` >= 0 (columns; lo may lie below the border column -1)
__host__ __device__ inline int extend_band_lo(int row, int w) { return row / kExtendBandBlockRows * kExtendBandBlockRows - w; }
__host__ __device__ inline int extend_band_hi(int row, int w) { return row / kExtendBandBlockRows * kExtendBandBlockRows + kExtendBandBlockRows - 1 + w; }

// The border column X(row, -1) / the border row X(-1, col) is a present cell
__host__ __device__ inline bool extend_band_border_col_present(int row, int w) { return row < 0 || extend_band_lo(row, w) <= -1; }
__host__ __device__ inline bool extend_band_border_row_present(int col, int w) { return col + 1 <= w; }

// Cell (row, col), row >= -1, col >= -1
__host__ __device__ inline bool extend_band_present(int row, int col, int w) {
    if (row < 0) return extend_band_border_row_present(col, w);
    return extend_band_lo(row, w) <= col && col <= extend_band_hi(row, w);
}

// The read end is unreached: row Rp - 1 has no present candidate -1 <= j < Fp
__host__ __device__ inline bool extend_band_unreached(int Rp, int Fp, int w) { return Rp > 0 && extend_band_lo(Rp - 1, w) > Fp - 1; }

// What strip `strip` (rows [512 strip, 512 strip + 512)) sweeps of a matrix of F columns: the columns [col_first, col_end) of the
// union of its lanes' windows, and the steps [t_begin, t_end) -- lane l sweeps column t - l at step t; t_begin is col_first
// rounded down to the 64-column blocks, t_end lets the last lane reach col_end - 1.  empty: no column below F.
struct ExtendBandStrip {
    bool empty;
    int col_first, col_end;
    int t_begin, t_end;
};
__host__ __device__ inline ExtendBandStrip extend_band_strip(int strip, int F, int w) {
    const int row0 = strip * kExtendBandStripRows;
    ExtendBandStrip s;
    const int lo = extend_band_lo(row0, w), hi = extend_band_hi(row0 + kExtendBandStripRows - 1, w);
    s.col_first = lo > 0 ? lo : 0;
    s.col_end = hi + 1 < F ? hi + 1 : F;
    s.empty = s.col_first >= s.col_end;
    s.t_begin = s.col_first / kExtendBandColAlign * kExtendBandColAlign;
    s.t_end = s.col_end + 63;
    return s;
}

// The last column the bottom row of the strip ABOVE strip `strip` > 0 holds a present cell in: the window's end of that strip's
// last block.  Beyond it the row above is absent -- and the boundary-row slot holds what an earlier strip left there.
__host__ __device__ inline int extend_band_top_hi(int strip, int w) { return extend_band_hi(strip * kExtendBandStripRows - 1, w); }

}  // namespace valign
