// subopt_kernels.hip.h -- the records of the suboptimal Smith-Waterman scores (include/valign_hip.h: valign_hip_subopt;
// engine_subopt.hip) behind the sweep that leaves the column maxima (placed_kernels.hip.h: score_placed_kernel<..., SUB = true>).
//
// A suboptimal score is the placed record plus score2 / ref_end2: the largest colmax[j] -- the maximum of column j over the rows
// below the pair's trimmed read length -- over the columns j below the trimmed reference length with |j - (ref_end - 1)| > mask,
// and the smallest such column that holds it.  The sweep wrote one row of dwords per pair of pairs, pair A in the low halves and
// pair B in the high halves; subopt_records_kernel gives a wave to each row: coalesced dword loads, the window and the tie rule
// per lane, one reduction.  It holds no DP.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "placed_kernels.hip.h"

namespace valign {

struct SuboptRec {            // = valign_hip_subopt (include/valign_hip.h), 20 bytes
    int score, read_end, ref_end, score2, ref_end2;
};

struct SuboptRecordArgs {
    const uint8_t *refs;      // n * F bytes, pair-major
    const PlacedRec *placed;  // n records of the sweep
    const unsigned *colmax;   // (n + 1) / 2 rows of col_stride dwords
    SuboptRec *subopt;        // n
    long long n;
    int F, col_stride, mask;
};

#ifdef VALIGN_TU_SUBOPT      // not a template: defined once, in engine_subopt.hip
__global__ void __launch_bounds__(256)
subopt_records_kernel(const SuboptRecordArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long pp = (long long)blockIdx.x * (256 / kWave) + threadIdx.x / kWave;      // wave-uniform
    if (2 * pp >= a.n) return;
    int trimmed[2], centre[2], score[2];
    PlacedRec rec[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const long long pair = 2 * pp + half;
        const bool there = pair < a.n;
        rec[half] = there ? a.placed[pair] : PlacedRec{0, 0, 0};
        // 1 + the position of the reference's last ACGT byte
        int len = 0;
        if (there) {
            const uint8_t *ref = a.refs + (size_t)pair * a.F;
            for (int j = lane; j < a.F; j += kWave) {
                const int c = base_class(ref[j]);
                if (c >= 1 && c <= 4) len = j + 1;
            }
        }
#pragma unroll
        for (int dd = kWave / 2; dd >= 1; dd >>= 1) {
            const int other = __shfl_xor(len, dd, kWave);
            len = other > len ? other : len;
        }
        // (the sweep stopped at the wave's last used column <= col_stride: nothing beyond the row is read whatever the bytes say)
        trimmed[half] = len < a.col_stride ? len : a.col_stride;
        score[half] = rec[half].score;
        centre[half] = rec[half].ref_end - 1;
    }
    const unsigned *row = a.colmax + (size_t)pp * a.col_stride;
    const int cols = trimmed[0] > trimmed[1] ? trimmed[0] : trimmed[1];
    int best[2] = {0, 0}, at[2] = {0, 0};           // a lane's columns ascend: a strictly greater value keeps the smallest column
    for (int j = lane; j < cols; j += kWave) {
        const unsigned v = row[j];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int val = (int)(half ? v >> 16 : v & 0xFFFFu);
            const int d = j - centre[half];
            const bool outside = (long long)(d < 0 ? -d : d) > (long long)a.mask;
            if (score[half] > 0 && j < trimmed[half] && outside && val > best[half]) {
                best[half] = val;
                at[half] = j + 1;
            }
        }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int dd = kWave / 2; dd >= 1; dd >>= 1) {
            const int ov = __shfl_xor(best[half], dd, kWave), oa = __shfl_xor(at[half], dd, kWave);
            if (ov > best[half] || (ov == best[half] && ov > 0 && oa < at[half])) {
                best[half] = ov;
                at[half] = oa;
            }
        }
        if (lane == half && 2 * pp + half < a.n) {
            SuboptRec r{0, 0, 0, 0, 0};
            if (score[half] > 0) {
                r.score = rec[half].score;
                r.read_end = rec[half].read_end;
                r.ref_end = rec[half].ref_end;
                r.score2 = best[half];
                r.ref_end2 = best[half] > 0 ? at[half] : 0;
            }
            a.subopt[2 * pp + half] = r;
        }
    }
}
#endif

}  // namespace valign
