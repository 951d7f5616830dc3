// band_window.h -- the block band of banded Smith-Waterman (include/valign_hip.h), one definition for the host and the device.
//
// The read's rows are taken in blocks of `block_rows` consecutive rows, the last block ending on the last row (so the first
// block holds `pad` = blocks * block_rows - R rows above row 0); every row of block b sweeps the columns
//   [floor(r_lo * F / R) - w, floor(r_hi * F / R) + w]  clipped to [0, F), the start rounded down to `col_align`,
// r_lo / r_hi the first / last real row of the block and w = band_half (oracle/cpu_ref.c, band_columns).  The banded
// alignment strips (strip_kernels.hip.h) force every other cell to 0 and sweep per strip the union of their rows' windows;
// traceback_kernel finds a strip's column offset from the same function.
#pragma once

#include "../../include/valign_hip.h"

#ifndef __HIPCC__       // plain g++ (the CPU checks of the plans that read the band): the functions below are host functions
#define __host__
#define __device__
#endif

namespace valign {

struct BandShape {
    int half;           // w; < 0: no band (every cell)
    int block_rows;     // B
    int col_align;      // A
    int pad;            // blocks * B - R
};

// Columns [lo, lo + width) of read row `row` (0-based; negative: a padding row above the matrix, which sweeps nothing).
__host__ __device__ inline void band_row_window(const BandShape &b, int row, int R, int F, int &lo, int &width) {
    if (b.half < 0) {
        lo = 0;
        width = F;
        return;
    }
    if (row < 0 || row >= R) {
        lo = 0;
        width = 0;
        return;
    }
    const int blk = (row + b.pad) / b.block_rows;
    int r_lo = blk * b.block_rows - b.pad, r_hi = r_lo + b.block_rows - 1;
    r_lo = r_lo < 0 ? 0 : r_lo;
    r_hi = r_hi > R - 1 ? R - 1 : r_hi;
    long long l = (long long)r_lo * F / R - b.half;
    const long long h = (long long)r_hi * F / R + b.half;
    l = l < 0 ? 0 : l;
    lo = (int)(l - l % b.col_align);
    width = (int)(h > F - 1 ? F - 1 : h) - lo + 1;
}

// Columns [c_lo, c_lo + width) swept by the rows [row_first, row_last] (real rows, ascending): the union of their windows
// (both ends of a window never decrease with the row).
__host__ __device__ inline void band_rows_window(const BandShape &b, int row_first, int row_last, int R, int F, int &c_lo, int &width) {
    int lo_last, w_last;
    band_row_window(b, row_first < 0 ? 0 : row_first, R, F, c_lo, width);
    band_row_window(b, row_last, R, F, lo_last, w_last);
    width = lo_last + w_last - c_lo;
}

// The score sweeps' strip band (score_long_kernel, long_kernels.hip.h): 160-row strips ARE the blocks, A = 4.
// Columns [c_lo, c_hi] swept by strip s.  c_lo is a multiple of 4 (16-byte ring accesses).
template <int G, int K>
__host__ __device__ inline void strip_columns(int s, int R, int F, int pad_rows, int band_half, int &c_lo, int &c_hi) {
    constexpr int rows = G * K;
    // (a band is only ever swept with the geometry whose strips are the API's blocks: Engine::score_long_device checks
    // G * K == VALIGN_HIP_BAND_BLOCK_ROWS there; taller strips exist for unbanded sweeps)
    static_assert(VALIGN_HIP_BAND_COL_ALIGN == 4, "c_lo is rounded down to a multiple of 4 below");
    if (band_half < 0 || R <= 0) {
        c_lo = 0;
        c_hi = F - 1;
        return;
    }
    int r_lo = s * rows - pad_rows, r_hi = (s + 1) * rows - pad_rows - 1;
    r_lo = r_lo < 0 ? 0 : r_lo;
    r_hi = r_hi > R - 1 ? R - 1 : r_hi;
    const long long lo = (long long)r_lo * F / R - band_half, hi = (long long)r_hi * F / R + band_half;
    c_lo = (int)(lo < 0 ? 0 : lo) & ~3;
    c_hi = (int)(hi > F - 1 ? F - 1 : hi);
}

}  // namespace valign
