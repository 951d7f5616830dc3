// placed_wide_kernels.hip.h -- placed Smith-Waterman scores on int32 cells (key placed_wide; include/valign_hip.h): the score
// of a pair and the cell its best local alignment ends in, for calls whose cells can leave int16 or that ask for
// score_width = 32 -- no pointer stream, no code arithmetic, no first_bad, no walk.
//
// score_placed_wide_kernel is the sweep of align_strip_wide_kernel<K, kAlgSW, AFFINE> (strip_kernels.hip.h) with everything
// that serves the traceback taken out: row strips of 64 K rows, one wave per pair-of-pairs and one launch per strip, the
// profile of the strip's rows and the ring of slab numbers in LDS (strip_ring_setup, fetch_profile), saturating subtracts on
// gap magnitudes, h_last / f_last handed to the next lane by a wave_shr DPP move, one int32 boundary row per pair (and an F
// row beside it for affine gaps) handed from strip to strip through two row sets that ping-pong (StripArgs.top / .bottom,
// the layout of align_strip_wide_kernel: set 2 * half (+ 1 for F) when affine, else set half; one set = top_f - top dwords).
// Per row a running best and the step of its first occurrence (strictly greater: the row's first column wins); after the
// sweep the wave reduces value, then smallest row, then that row's column, and merges into EndCell -- the high half of the
// value in EndCell.pad -- where a later strip wins only with a strictly larger value: the row-major first maximum of the
// reference (src/Kernels/default/DefaultKernel.cpp:252-256).
//
// ONE pass over the strip for both pairs of the wave (align_strip_wide_kernel sweeps twice, pair A then pair B): the two int32
// chains of a lane are independent, so each fills the other's latency slots, and the profile fetch, the ring refill, the loop
// control and the column mask are paid once per step instead of twice.  DESIGN.md (section 3) has the registers and the
// hot-loop histogram.
#pragma once

#include "placed_kernels.hip.h"
#include "strip_kernels.hip.h"

namespace valign {

// The int32 value of an end cell written by the int32 sweeps: EndCell.pad is the high half
__device__ __forceinline__ int end_cell_wide_score(const EndCell e) {
    return (int)((unsigned)(unsigned short)e.score | ((unsigned)(unsigned short)e.pad << 16));
}

template <int K, bool AFFINE>
__global__ void __launch_bounds__(64)
score_placed_wide_kernel(const StripArgs args) {
    constexpr int G = 64;
    constexpr int kSets = AFFINE ? 2 : 1;                 // boundary row sets per pair
    using geo = Geo<G, K>;
    const int lane = threadIdx.x;
    const int l = lane;
    const int R = args.R, F = args.F;
    const int pad_total = args.strips * geo::kRows - R;
    const int row0 = args.strip * geo::kRows - pad_total;
    const int strip_pad = args.strip * geo::kRows;

    WaveTables w;
    if (!strip_ring_setup<K>(args.reads, args.n, R, F, args.match, args.mismatch, row0, w)) return;
    const unsigned lane_base = lds_offset(w.prof) + l * geo::kLaneBytes;
    const unsigned ring_base = lds_offset(w.refc);
    const uint8_t *ref_a = args.refs + w.pair0 * F, *ref_b = args.refs + (w.pair0 + (w.last >= 1 ? 1 : 0)) * F;
    // magnitudes for the floor-at-zero subtract
    const unsigned g_read = (unsigned)-args.gap_read, g_ref = (unsigned)-args.gap_ref;
    const unsigned o_read = (unsigned)-args.open_read, e_read = (unsigned)-args.ext_read;
    const unsigned o_ref = (unsigned)-args.open_ref, e_ref = (unsigned)-args.ext_ref;
    auto sub0 = [](int v, unsigned c) __attribute__((always_inline)) { return (int)__builtin_elementwise_sub_sat((unsigned)v, c); };
    auto max2 = [](int a, int b) __attribute__((always_inline)) { return a > b ? a : b; };
    const long long pp = w.pair0 / 2;
    const size_t set_dwords = (size_t)(args.top_f - args.top);
    const bool has_top = args.strip > 0, has_bottom = args.strip + 1 < args.strips;
    const int steps = F + G - 1;
    const int row_dwords = args.row_dwords;
    const unsigned *top[2], *top_f[2];
    unsigned *bottom[2], *bottom_f[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        top[half] = args.top + (size_t)(kSets * half) * set_dwords + pp * row_dwords;
        bottom[half] = args.bottom + (size_t)(kSets * half) * set_dwords + pp * row_dwords;
        top_f[half] = top[half] + set_dwords;             // (affine only)
        bottom_f[half] = bottom[half] + set_dwords;
    }

    int Hl[2][K], El[2][AFFINE ? K : 1];
    int rb[2][K], fc[2][K];                               // per row: the best value and the step of its first occurrence
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int q = 0; q < K; ++q) {
            Hl[half][q] = 0;
            if (AFFINE) El[half][q] = 0;
            rb[half][q] = 0;
            fc[half][q] = 0;
        }
    }
    int h_last[2] = {0, 0}, f_last[2] = {0, 0}, up0[2] = {0, 0};
    unsigned top_cur[2] = {0u, 0u}, top_next[2], topf_cur[2] = {0u, 0u}, topf_next[2] = {0u, 0u};
    unsigned bot_acc[2] = {0u, 0u}, botf_acc[2] = {0u, 0u};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        top_next[half] = has_top ? top[half][lane] : 0u;
        if (AFFINE) topf_next[half] = has_top ? top_f[half][lane] : 0u;
    }
    int j = -l;
    unsigned code_addr = ring_base | ((unsigned)(-2 * l) & (2u * kStripRingCols - 1u));
    StripRefBytes ref_raw = strip_ring_request(ref_a, ref_b, lane, F);     // columns [0, 64)

    for (int t = 0; t < steps; ++t) {
        if ((t & 63) == 0) {
            const bool more = has_top && t + 64 + lane < row_dwords;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                top_cur[half] = top_next[half];
                top_next[half] = more ? top[half][t + 64 + lane] : 0u;
                if (AFFINE) {
                    topf_cur[half] = topf_next[half];
                    topf_next[half] = more ? top_f[half][t + 64 + lane] : 0u;
                }
            }
            strip_ring_commit<K>(w.refc, t + lane, F, ref_raw);
            ref_raw = strip_ring_request(ref_a, ref_b, t + 64 + lane, F);
        }
        int diag0[2], fup0[2] = {0, 0};
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            diag0[half] = up0[half];
            // every lane takes part in the DPP move, before the select on the lane's column
            const int above = __builtin_amdgcn_readlane((int)top_cur[half], t & 63);
            int from_lane = __builtin_amdgcn_update_dpp(0, h_last[half], 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
            asm volatile("" : "+v"(from_lane));
            up0[half] = l == 0 ? above : from_lane;
            if (AFFINE) {
                const int above_f = __builtin_amdgcn_readlane((int)topf_cur[half], t & 63);
                int f_lane = __builtin_amdgcn_update_dpp(0, f_last[half], 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
                asm volatile("" : "+v"(f_lane));
                fup0[half] = l == 0 ? above_f : f_lane;
            }
        }
        if ((unsigned)j < (unsigned)F) {
            const unsigned ca = *(lds_cu8 *)(code_addr), cb = *(lds_cu8 *)(code_addr + 1);
            s16x2 S[K];
            fetch_profile<G, K>(lane_base + ca * geo::kPairStride, lane_base + cb * geo::kPairStride, S);
            int h[2] = {up0[0], up0[1]}, f[2] = {fup0[0], fup0[1]};
            int d_cur[2] = {diag0[0] + (int)S[0].x, diag0[1] + (int)S[0].y};
#pragma unroll
            for (int q = 0; q < K; ++q) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {             // two independent chains: pair A, pair B
                    int d_next = 0;
                    if (q + 1 < K) d_next = Hl[half][q] + (int)(half ? S[q + 1].y : S[q + 1].x);      // before Hl[q] is overwritten
                    int m;
                    if constexpr (AFFINE) {
                        const int e = max2(sub0(El[half][q], e_read), sub0(Hl[half][q], o_read));
                        El[half][q] = e;
                        f[half] = max2(sub0(f[half], e_ref), sub0(h[half], o_ref));
                        m = max2(max2(d_cur[half], e), f[half]);
                    } else {
                        m = max2(d_cur[half], max2(sub0(Hl[half][q], g_read), sub0(h[half], g_ref)));
                    }
                    h[half] = m;
                    Hl[half][q] = m;
                    d_cur[half] = d_next;
                    if (m > rb[half][q]) {                         // strictly greater: the first arg-max of the row wins
                        rb[half][q] = m;
                        fc[half][q] = t;
                    }
                }
            }
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                h_last[half] = h[half];
                f_last[half] = f[half];
            }
        }
        if (has_bottom) {
            const int col = t - (G - 1);
            if (col >= 0) {
                const bool mine = lane == (col & 63), flush = (col & 63) == 63 || t == steps - 1;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int v = __builtin_amdgcn_readlane(h_last[half], G - 1);
                    bot_acc[half] = mine ? (unsigned)v : bot_acc[half];
                    if (flush) bottom[half][(col & ~63) + lane] = bot_acc[half];
                    if (AFFINE) {
                        const int vf = __builtin_amdgcn_readlane(f_last[half], G - 1);
                        botf_acc[half] = mine ? (unsigned)vf : botf_acc[half];
                        if (flush) bottom_f[half][(col & ~63) + lane] = botf_acc[half];
                    }
                }
            }
        }
        ++j;
        code_addr = ((code_addr + 2u) & (2u * kStripRingCols - 1u)) | ring_base;
    }

    // ---- end cells: the largest value, then the smallest row, then the row's first column; over the strips, a later one only
    // wins with a larger value ----
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const long long pair = w.pair0 + half;
        int bv = 0, bq = 0, bcol = 0;
#pragma unroll
        for (int q = 0; q < K; ++q) {
            if (rb[half][q] > bv) {
                bv = rb[half][q];
                bq = q;
                bcol = fc[half][q];
            }
        }
        int vmax = bv;
#pragma unroll
        for (int dd = G / 2; dd >= 1; dd >>= 1) {
            const int other = __shfl_xor(vmax, dd, kWave);
            vmax = other > vmax ? other : vmax;
        }
        int p = bv == vmax ? l * K + bq : 0x7FFFFFFF;
#pragma unroll
        for (int dd = G / 2; dd >= 1; dd >>= 1) {
            const int other = __shfl_xor(p, dd, kWave);
            p = other < p ? other : p;
        }
        const int win_lane = p / K;
        const int col_t = __shfl(bcol, win_lane, kWave);
        EndCell out;
        out.score = (short)(vmax & 0xFFFF);
        out.pad = (short)((unsigned)vmax >> 16);
        out.read_pos = (short)(strip_pad + p - pad_total);
        out.ref_pos = (short)(col_t - win_lane);
        if (vmax <= 0) {
            out.read_pos = 0;
            out.ref_pos = 0;
        }
        if (l == 0 && pair < args.n) {
            if (args.strip == 0 || vmax > end_cell_wide_score(args.ends[pair])) args.ends[pair] = out;
        }
    }
}

#ifdef VALIGN_TU_PLACED      // not a template: defined once, in engine_placed.hip
// The int32 sweep's end cells -> records: the value is pad : score, and does not saturate
__global__ void __launch_bounds__(256)
placed_wide_records_kernel(const EndCell *ends, PlacedRec *placed, long long n) {
    const long long pair = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pair >= n) return;
    const EndCell e = ends[pair];
    const int v = end_cell_wide_score(e);
    const bool hit = v > 0;
    PlacedRec r;
    r.score = hit ? v : 0;
    r.read_end = hit ? (int)e.read_pos + 1 : 0;
    r.ref_end = hit ? (int)e.ref_pos + 1 : 0;
    placed[pair] = r;
}
#endif

}  // namespace valign
