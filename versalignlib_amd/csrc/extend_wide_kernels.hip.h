// extend_wide_kernels.hip.h -- extension scores on int32 cells and row strips (key extend_wide; include/valign_hip.h): the anchored
// score, its end cell and the read-end score (extend_kernels.hip.h has the matrix, tests/extend_ref.py restates it) for the calls
// the packed int16 register sweep refuses -- score_width = 32, cells that can leave int16, reads of more than 1 024 rows.
//
// score_extend_wide_kernel is score_placed_wide_kernel (placed_wide_kernels.hip.h) on the extension's matrix.  Kept: one wave per
// pair-of-pairs and one launch per strip of 64 K rows, both int32 chains of a lane in ONE pass, the profile of the strip's rows and
// the ring of slab numbers in LDS (strip_ring_setup, fetch_profile), the wave_shr hand-over of h_last / f_last, the boundary row
// sets that ping-pong from strip to strip (StripArgs.top / .bottom, the layout of score_placed_wide_kernel), a first arg-max per
// row and the reduction value -> smallest row -> that row's first column.  What differs is the matrix:
//   * no floor: plain signed adds of the gap scores (all <= 0) and signed maxima; extend_int32_ok (cell_rules.h) vouches for the
//     range and for the sentinel kExtendWideLoses that stands for the gap states of the two borders.
//   * the read sits TOP-aligned: strip s holds the read positions [s * 64 K, (s + 1) * 64 K), the padding rows lie below the
//     read in the last strip.  A padding row above row 0 could not reproduce a gap-priced border row; below the read nothing
//     reads one, and strip_ring_setup scores rows at or beyond R as 0.  (A padding row's border value is that of row R - 1.)
//   * the border column X(i, -1) = open_ref + i ext_ref (linear: (i + 1) gap_ref) in closed form, in every strip: each row's Hl
//     (the LEFT and DIAG input of column 0), up0 of the lane's first row (X(-1, -1) = 0 above row 0 of strip 0), h_last (what the
//     lane behind receives while this lane has not started), and the row's running best rb with fc = the step at which the lane
//     would sweep column -1 -- so that the border column is candidate 0 of the read-end score.  E starts at the sentinel.
//   * the border row X(-1, j) = open_read + j ext_read in strip 0: lane 0's `above` of step t, wave-uniform -- one running add on
//     the scalar unit -- with the sentinel as its F; later strips read the boundary rows as the placed sweep does.
//   * trimmed lengths Rp, Fp (1 + the position of the last ACGT byte) per pair, wave-uniform, from extend_wide_lengths_kernel,
//     which runs once per chunk: a row tracks column j only while j < Fp of ITS pair.  Columns at or beyond the larger Fp of the
//     wave are candidates of nothing and feed no candidate: the sweep ends there; a strip wholly below both reads' Rp returns.
//   * records across strips: a partial record per pair (five dwords, StripArgs.ptr) -- score / read_end / ref_end merged strip
//     after strip, a later strip winning only with a strictly larger value (the row-major first maximum, as EndCell is merged by
//     score_placed_wide_kernel), gscore / gref_end written by the strip and lane that hold row Rp - 1 from that row's rb / fc.
//     extend_wide_records_kernel copies them out and applies the definition's last empty case, Rp = 0: five zeros (score <= 0:
//     three zeros is what the merge leaves).  Values and coordinates are int32 from the cell to the record: nothing saturates.
// A short read fills a fraction of its one 512-row strip (as on the placed int32 sweep): the int16 register sweep is the route for
// those wherever the rule lets it run.  Z-drop, a band around the anchor's diagonal and an end bonus are not built.
// (Since then the band IS built, on this strip sweep: the BANDED instances, below.  Z-drop and an end bonus remain unbuilt.)
// (And since then a row-wise Z-drop IS built: the ZDROP instances, further below.)
//
// BANDED (key extend_band; the band is extend_band_plan.h's, StripArgs.band.half its w): the same sweep over the present cells
// only.  A lane's 8 rows are one block of the band, so a lane is wholly inside or wholly outside its window at any step and the
// mask costs per step, not per cell:
//   * outside its window a lane updates nothing; past the window it hands kExtendWideLoses down as h_last (and f_last): the lane
//     behind then sees an ABSENT row above, and one step later an absent diagonal;
//   * a lane whose border column is absent starts with Hl = El = the sentinel (the absent LEFT and DIAG inputs of its window's
//     first column), h_last = the sentinel, and every row's rb at "no candidate" (INT32_MIN, which is the record's
//     VALIGN_HIP_EXTEND_UNREACHED); the diagonal input of its first row comes from the hand-over of the step before, which the
//     DPP move delivers while the lane is idle.  A lane whose border column is present starts as on the unbanded sweep;
//   * the step loop covers the strip's window only, [t_begin, t_end) of extend_band_strip: the ring requests, the boundary-row
//     reads and the bottom-row flushes start at t_begin, a multiple of 64.
// Four places that go wrong silently:
//   STALE BOUNDARY-ROW COLUMNS  a strip writes its bottom row over its own window only and the slots ping-pong, so the columns
//     beside it hold what the strip two above left there.  The strip below takes `above` (and the F row's) as the sentinel for
//     every column beyond extend_band_top_hi -- the window's end of the last block above -- whatever the slot holds there.
//   BORDER ROW  X(-1, j) is absent for j >= w: strip 0's `lead` is replaced by the sentinel there.
//   EMPTY WINDOW  a strip > 0 whose window has no column below the larger Fp returns before its set-up (so does every strip
//     below it: the windows move right).  Strip 0 never returns early: it initialises the partial records, so the merge of a
//     later strip never reads rec[0] uninitialised.
//   UNREACHED READ END  the lane that holds row Rp - 1 writes (INT32_MIN, 0) when the row had no candidate; where that strip
//     returned early nobody writes the pair, and extend_wide_records_kernel puts the closed form (extend_band_unreached) there.
//
// ZDROP (key extend_zdrop; the rule, its step, its combine and the skip condition are extend_zdrop.h's): no cell changes, only which
// rows count.  The row maxima rb / fc the sweep keeps in registers are all the rule reads, so everything happens at the two ends:
//   * per pair one more int of state behind the trimmed lengths: the drop row T (kExtendZdropNone: not dropped).  The three
//     scratch arrays -- records, lengths, drop rows -- lie one behind the other, each sized for the same pair count, which is how
//     the kernel finds the third from the two pointers it is given.  The running best is the partial record's first three ints.
//   * entry: behind the early returns above, a strip > 0 whose two pairs both dropped above it returns before its set-up and one
//     lane counts the wave (StripArgs.walk carries the engine's counter dword; StripArgs.band.pad carries Z: this sweep has no
//     padding rows above the read).  Strip 0 always runs and starts the state.
//   * epilogue, in the place of the value -> row -> column reduction: each lane's rows in order, an exclusive prefix arg-max over
//     the lanes seeded with the carried running best (wave shuffles: the maxima never leave the wave), each lane's walk to its first
//     dropping row, a wave minimum for T; the lane that holds T writes the running best just before it and T, without a drop lane
//     63 writes the inclusive total.  A pair that entered the strip dropped writes nothing.
// The closing kernels make the read end of a dropped pair unreached (T < Rp).
#pragma once

#include "extend_band_align_plan.h"
#include "extend_band_plan.h"
#include "extend_kernels.hip.h"
#include "extend_zdrop.h"
#include "strip_kernels.hip.h"

namespace valign {

constexpr int kExtendWideK = 8;                 // rows per lane: the K of the placed int32 sweep
constexpr int kExtendWideRecDwords = 5;         // a partial record: ExtendRec's five ints
static_assert(sizeof(ExtendRec) == 4 * kExtendWideRecDwords, "the partial record is an ExtendRec");

// ZDROP: the drop rows of a chunk lie behind its trimmed lengths as those lie behind its partial records, all three sized for the same
// pair count -- (first_bad - ptr) / 5 pairs
__host__ __device__ inline int *extend_drop_rows(const StripArgs &a) {
    const long long slots = (a.first_bad - reinterpret_cast<const int *>(a.ptr)) / kExtendWideRecDwords;
    return const_cast<int *>(a.first_bad) + 2 * slots;
}

// StripArgs of this sweep: ptr = the partial records (n x 5 dwords), first_bad = the trimmed lengths (n x 2: Rp, Fp); ends unused.
// PTRS (BANDED only; extend_band_align_kernels.hip.h names the instances and has the codes): the sweep also derives every cell's
// back pointer and streams the codes to StripArgs.ends, taken as the dwords of the chunk's pointer regions in the layout of
// extend_band_align_plan.h.  Everything PTRS adds stands under `if constexpr (PTRS)`: the score instances compile to the
// instructions they had without it.
// ZDROP (above) is the last parameter and false by default; everything it adds stands under `if constexpr (ZDROP)`, so the six
// instances of the parameter list as it stood -- template <int K, bool AFFINE, bool BANDED = false, bool PTRS = false> -- compile to
// the instructions they had.
template <int K, bool AFFINE, bool BANDED = false, bool PTRS = false, bool ZDROP = false>
__global__ void __launch_bounds__(64)
score_extend_wide_kernel(const StripArgs args) {
    static_assert(!BANDED || K == kExtendBandBlockRows, "a lane's rows are one block of the band");
    static_assert(!PTRS || BANDED, "the pointer stream is the banded sweep's");
    constexpr int G = 64;
    constexpr int kSets = AFFINE ? 2 : 1;                 // boundary row sets per pair
    constexpr int kLoses = kExtendWideLoses;
    using geo = Geo<G, K>;
    const int lane = threadIdx.x;
    const int l = lane;
    const int R = args.R;
    const int row0 = args.strip * geo::kRows;             // top-aligned: the read position of the strip's first row

    // ---- trimmed lengths of the wave's two pairs (wave-uniform) ----
    const long long first_pair = (long long)blockIdx.x * geo::kPairs;
    if (first_pair >= args.n) return;
    int Rp[2], Fp[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const long long pair = first_pair + half < args.n ? first_pair + half : first_pair;
        Rp[half] = __builtin_amdgcn_readfirstlane(args.first_bad[2 * pair]);
        Fp[half] = __builtin_amdgcn_readfirstlane(args.first_bad[2 * pair + 1]);
    }
    // rows at or beyond Rp are no candidates and nothing above them reads them: strip 0 always runs (it starts the records)
    if (args.strip > 0 && (Rp[0] > Rp[1] ? Rp[0] : Rp[1]) <= row0) return;
    // columns at or beyond the larger Fp: tracked by neither pair, read by no column before them
    const int F = Fp[0] > Fp[1] ? Fp[0] : Fp[1];
    // BANDED: the strip's window.  EMPTY WINDOW: strip > 0 returns here, before the set-up; strip 0 goes on (it starts the records)
    const int bw = BANDED ? args.band.half : 0;
    const ExtendBandStrip win = extend_band_strip(args.strip, F, bw);
    if (BANDED && args.strip > 0 && win.empty) return;
    const int t_begin = BANDED ? win.t_begin : 0;
    // ZDROP: the drop rows lie behind the lengths as the lengths lie behind the records; both pairs dropped above the strip: skipped
    int *drop_rows = nullptr;
    int T_in[2] = {kExtendZdropNone, kExtendZdropNone};
    if constexpr (ZDROP) {
        drop_rows = extend_drop_rows(args);
        if (args.strip > 0) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const long long pair = first_pair + half < args.n ? first_pair + half : first_pair;
                T_in[half] = __builtin_amdgcn_readfirstlane(drop_rows[pair]);
            }
            if (extend_zdrop_strip_skipped(args.strip, T_in[0], T_in[1])) {
                if (lane == 0) atomicAdd(reinterpret_cast<unsigned *>(const_cast<WalkState *>(args.walk)), 1u);
                return;
            }
        }
    }

    WaveTables w;
    if (!strip_ring_setup<K>(args.reads, args.n, R, F, args.match, args.mismatch, row0, w)) return;
    const unsigned lane_base = lds_offset(w.prof) + l * geo::kLaneBytes;
    const unsigned ring_base = lds_offset(w.refc);
    const uint8_t *ref_a = args.refs + w.pair0 * args.F, *ref_b = args.refs + (w.pair0 + (w.last >= 1 ? 1 : 0)) * args.F;
    // the scores themselves, all <= 0: added
    const int g_read = args.gap_read, g_ref = args.gap_ref;
    const int o_read = args.open_read, e_read = args.ext_read;
    const int o_ref = args.open_ref, e_ref = args.ext_ref;
    auto max2 = [](int a, int b) __attribute__((always_inline)) { return a > b ? a : b; };
    // X(i, -1): a gap of i + 1 read bases against nothing; X(-1, -1) = 0; padding rows as row R - 1
    auto border_col = [&](int row) __attribute__((always_inline)) -> int {
        const int i = row < R ? row : R - 1;
        if (i < 0) return 0;
        return AFFINE ? o_ref + i * e_ref : (i + 1) * g_ref;
    };
    const long long pp = w.pair0 / 2;
    const size_t set_dwords = (size_t)(args.top_f - args.top);
    const bool has_top = args.strip > 0, has_bottom = args.strip + 1 < args.strips;
    const int steps = BANDED ? win.t_end : F + G - 1;         // the step loop ends here
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
    int h_last[2], f_last[2], up0[2];
    // BANDED: the lane's window [j_lo, j_hi] (j_lo may lie below column 0) and whether its border column is a present cell
    const int j_lo = BANDED ? extend_band_lo(row0 + l * K, bw) : 0, j_hi = BANDED ? extend_band_hi(row0 + l * K, bw) : 0;
    const bool edge = !BANDED || extend_band_border_col_present(row0 + l * K, bw);
    const bool edge_above = !BANDED || extend_band_border_col_present(row0 + l * K - 1, bw);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int q = 0; q < K; ++q) {
            Hl[half][q] = edge ? border_col(row0 + l * K + q) : kLoses;
            if (AFFINE) El[half][q] = kLoses;
            rb[half][q] = edge ? Hl[half][q] : (int)0x80000000;       // the row's best so far: column -1 (BANDED, absent: no candidate) ...
            fc[half][q] = l - 1;                          // ... which this lane would sweep at step l - 1
        }
        up0[half] = edge_above ? border_col(row0 + l * K - 1) : kLoses;
        h_last[half] = edge ? border_col(row0 + l * K + K - 1) : kLoses;
        f_last[half] = kLoses;
        // BANDED, a window that starts beyond column 0: lane 0's first diagonal input is the column before the first 64-column
        // block of the row above (inside the window of the last block above; strip 0's window starts at column 0)
        if (BANDED && t_begin > 0 && l == 0) up0[half] = has_top ? (int)top[half][t_begin - 1] : kLoses;
    }
    // STALE BOUNDARY-ROW COLUMNS: the last column the row above is present in; beyond it `above` is the sentinel, not the slot
    const int top_hi = BANDED ? extend_band_top_hi(args.strip > 0 ? args.strip : 1, bw) : 0;
    unsigned top_cur[2] = {0u, 0u}, top_next[2], topf_cur[2] = {0u, 0u}, topf_next[2] = {0u, 0u};
    unsigned bot_acc[2] = {0u, 0u}, botf_acc[2] = {0u, 0u};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        top_next[half] = has_top ? top[half][t_begin + lane] : 0u;
        if (AFFINE) topf_next[half] = has_top ? top_f[half][t_begin + lane] : 0u;
    }
    // the border row of strip 0: X(-1, t) and what a step adds to it (wave-uniform)
    int lead = AFFINE ? o_read : g_read;
    const int lead_step = AFFINE ? e_read : g_read;
    int j = BANDED ? t_begin - l : -l;
    unsigned code_addr = ring_base | ((unsigned)(BANDED ? 2 * (t_begin - l) : -2 * l) & (2u * kStripRingCols - 1u));
    StripRefBytes ref_raw = strip_ring_request(ref_a, ref_b, t_begin + lane, F);     // columns [0, 64) (BANDED: from t_begin)
    // PTRS: a dword per row, pair A's codes in the low half, pair B's in the high half, 2 bits per step, the newest lowest; and
    // the lane's first dword of the strip's first block (the regions are sized for the engine's F: args.F)
    unsigned acc_h[PTRS ? K : 1], acc_g[PTRS && AFFINE ? K : 1];
    unsigned *stream = nullptr;
    if constexpr (PTRS) {
#pragma unroll
        for (int q = 0; q < K; ++q) {
            acc_h[q] = 0u;
            if (AFFINE) acc_g[q] = 0u;
        }
        stream = reinterpret_cast<unsigned *>(args.ends) + pp * extend_band_align_pp_dwords(R, args.F, bw, AFFINE) +
                 extend_band_align_strip_base(args.strip, args.F, bw, AFFINE) + extend_band_align_word(0, l, 0, AFFINE);
    }

    for (int t = t_begin; t < steps; ++t) {
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
            int above = has_top ? __builtin_amdgcn_readlane((int)top_cur[half], t & 63) : lead;
            // BANDED: absent above -- beyond the last block's window of the strip above (STALE BOUNDARY-ROW COLUMNS), or the
            // BORDER ROW from column w on
            if (BANDED) above = (has_top ? t <= top_hi : t < bw) ? above : kLoses;
            int from_lane = __builtin_amdgcn_update_dpp(0, h_last[half], 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
            asm volatile("" : "+v"(from_lane));
            up0[half] = l == 0 ? above : from_lane;
            if (AFFINE) {
                int above_f = has_top ? __builtin_amdgcn_readlane((int)topf_cur[half], t & 63) : kLoses;
                if (BANDED) above_f = t <= top_hi ? above_f : kLoses;       // (the F row's stale columns)
                int f_lane = __builtin_amdgcn_update_dpp(0, f_last[half], 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
                asm volatile("" : "+v"(f_lane));
                fup0[half] = l == 0 ? above_f : f_lane;
            }
        }
        lead += lead_step;
        if constexpr (PTRS) {       // every step in every lane, so that bit positions depend on the step alone; each half drops its oldest code
#pragma unroll
            for (int q = 0; q < K; ++q) {
                acc_h[q] = (acc_h[q] << 2) & 0xFFFCFFFCu;
                if (AFFINE) acc_g[q] = (acc_g[q] << 2) & 0xFFFCFFFCu;
            }
        }
        if ((unsigned)j < (unsigned)F && (!BANDED || (j >= j_lo && j <= j_hi))) {
            const unsigned ca = *(lds_cu8 *)(code_addr), cb = *(lds_cu8 *)(code_addr + 1);
            s16x2 S[K];
            fetch_profile<G, K>(lane_base + ca * geo::kPairStride, lane_base + cb * geo::kPairStride, S);
            const bool in_cols[2] = {j < Fp[0], j < Fp[1]};       // the column is one of the pair's own
            int h[2] = {up0[0], up0[1]}, f[2] = {fup0[0], fup0[1]};
            int d_cur[2] = {diag0[0] + (int)S[0].x, diag0[1] + (int)S[0].y};
#pragma unroll
            for (int q = 0; q < K; ++q) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {             // two independent chains: pair A, pair B
                    int d_next = 0;
                    if (q + 1 < K) d_next = Hl[half][q] + (int)(half ? S[q + 1].y : S[q + 1].x);      // before Hl[q] is overwritten
                    int m;
                    if constexpr (PTRS) {
                        // the equality tests of align_extend_fill_kernel on int32 cells; a sentinel-derived candidate equals no cell
                        const int d = d_cur[half];
                        unsigned code;
                        if constexpr (AFFINE) {
                            const int e_open = Hl[half][q] + o_read, f_open = h[half] + o_ref;
                            const int e = max2(El[half][q] + e_read, e_open);
                            El[half][q] = e;
                            f[half] = max2(f[half] + e_ref, f_open);
                            m = max2(max2(d, e), f[half]);
                            // bit 0: the vertical state was extended, bit 1: the horizontal one -- an open wins a tie
                            const unsigned gap = (f[half] != f_open ? 1u : 0u) | (e != e_open ? 2u : 0u);
                            acc_g[q] |= gap << (16 * half);
                            code = m == d ? 0u : (m == f[half] ? 1u : 2u);      // DIAG before the vertical before the horizontal state
                        } else {
                            const int up = h[half] + g_ref;
                            m = max2(d, max2(Hl[half][q] + g_read, up));
                            code = m == d ? 0u : (m == up ? 1u : 2u);           // DIAG before UP before LEFT
                        }
                        acc_h[q] |= code << (16 * half);
                    } else if constexpr (AFFINE) {
                        const int e = max2(El[half][q] + e_read, Hl[half][q] + o_read);
                        El[half][q] = e;
                        f[half] = max2(f[half] + e_ref, h[half] + o_ref);
                        m = max2(max2(d_cur[half], e), f[half]);
                    } else {
                        m = max2(d_cur[half], max2(Hl[half][q] + g_read, h[half] + g_ref));
                    }
                    h[half] = m;
                    Hl[half][q] = m;
                    d_cur[half] = d_next;
                    if (m > rb[half][q] && in_cols[half]) {        // strictly greater: the first arg-max of the row wins
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
        if (BANDED && j > j_hi) {          // past the window: the row above the lane behind is absent from here on
            h_last[0] = h_last[1] = kLoses;
            f_last[0] = f_last[1] = kLoses;
        }
        if constexpr (PTRS) {
            // a block every 8 steps from t_begin (a multiple of 64); the strip's last block is stored even when it holds fewer
            // steps, its codes moved up to the positions of a whole block
            const int in_block = t & (kExtendBandAlignBlockSteps - 1);
            if (in_block == kExtendBandAlignBlockSteps - 1 || t == steps - 1) {
                const int up = 2 * (kExtendBandAlignBlockSteps - 1 - in_block);
                const unsigned keep = ~(((1u << up) - 1u) << 16);                // what pair A's half would push into pair B's
                uint4 *block = reinterpret_cast<uint4 *>(stream + extend_band_align_word((t - t_begin) / kExtendBandAlignBlockSteps, 0, 0, AFFINE));
#pragma unroll
                for (int q = 0; q < K; q += 4)
                    block[q / 4] = uint4{(acc_h[q] << up) & keep, (acc_h[q + 1] << up) & keep, (acc_h[q + 2] << up) & keep, (acc_h[q + 3] << up) & keep};
                if constexpr (AFFINE) {
#pragma unroll
                    for (int q = 0; q < K; q += 4)
                        block[(K + q) / 4] = uint4{(acc_g[q] << up) & keep, (acc_g[q + 1] << up) & keep, (acc_g[q + 2] << up) & keep, (acc_g[q + 3] << up) & keep};
                }
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

    // ---- the partial records.  Anchored score: the largest value > 0, then the smallest row, then the row's first column; over
    // the strips, a later one only wins with a larger value.  Read-end score: row Rp - 1's own entry, the border column included ----
    int *partial = reinterpret_cast<int *>(args.ptr);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const long long pair = w.pair0 + half;
        if constexpr (ZDROP) {
            if (pair >= args.n || T_in[half] < row0) continue;        // no such pair, or it entered the strip dropped: nothing is written
            int *rec = partial + kExtendWideRecDwords * pair;
            const int Z = args.band.pad;
            const int price_ref = extend_zdrop_price(AFFINE ? e_ref : g_ref), price_read = extend_zdrop_price(AFFINE ? e_read : g_read);
            // the carried running best (read by every lane before any lane writes it)
            ExtendZdropBest seed = extend_zdrop_anchor();
            if (args.strip > 0) seed = extend_zdrop_from_record(rec[0], rec[1], rec[2]);
            const int first_row = row0 + l * K;
            // 1. the lane's rows in order: rows of the read that have a candidate
            ExtendZdropBest mine = extend_zdrop_no_row();
#pragma unroll
            for (int q = 0; q < K; ++q)
                if (first_row + q < Rp[half] && rb[half][q] != (int)0x80000000)
                    mine = extend_zdrop_combine(mine, ExtendZdropBest{rb[half][q], first_row + q, fc[half][q] - l});
            // 2. the exclusive prefix over the lanes, seeded
            ExtendZdropBest run = mine;
#pragma unroll
            for (int dd = 1; dd < G; dd <<= 1) {
                const ExtendZdropBest before{__shfl_up(run.m, dd, kWave), __shfl_up(run.i, dd, kWave), __shfl_up(run.j, dd, kWave)};
                if (l >= dd) run = extend_zdrop_combine(before, run);
            }
            const ExtendZdropBest upto{__shfl_up(run.m, 1, kWave), __shfl_up(run.i, 1, kWave), __shfl_up(run.j, 1, kWave)};
            ExtendZdropBest best = l == 0 ? seed : extend_zdrop_combine(seed, upto);
            // 3. the lane's walk: its first dropping row; the running best stays as it was just before that row
            int T = kExtendZdropNone;
#pragma unroll
            for (int q = 0; q < K; ++q) {
                if (T == kExtendZdropNone && first_row + q < Rp[half] && rb[half][q] != (int)0x80000000 &&
                    extend_zdrop_step(best, first_row + q, rb[half][q], fc[half][q] - l, Z, price_ref, price_read))
                    T = first_row + q;
            }
            int T_wave = T;
#pragma unroll
            for (int dd = G / 2; dd >= 1; dd >>= 1) {
                const int other = __shfl_xor(T_wave, dd, kWave);
                T_wave = other < T_wave ? other : T_wave;
            }
            // 4. the running best just before T, from the lane that holds T; without a drop the inclusive total, from the last lane
            if (T_wave != kExtendZdropNone ? T == T_wave : l == G - 1) {
                rec[0] = best.m;
                rec[1] = best.i + 1;                      // half-open ends; the anchor is three zeros
                rec[2] = best.j + 1;
                drop_rows[pair] = T_wave;
            }
            // 5. the read-end score, as without the key (the closing kernel makes it unreached where T < Rp)
            const int last_row = Rp[half] - 1 - row0;
            if (last_row >= 0 && last_row < geo::kRows && last_row / K == l) {
                int gs = 0, gt = 0;
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    if (q == last_row % K) {
                        gs = rb[half][q];
                        gt = fc[half][q];
                    }
                }
                rec[3] = gs;
                rec[4] = gt - l + 1;
            }
            continue;
        }
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
        if (pair >= args.n) continue;
        int *rec = partial + kExtendWideRecDwords * pair;
        if (l == 0) {
            const bool hit = vmax > 0;
            if (args.strip == 0 || vmax > rec[0]) {       // (rec[0] >= 0 once strip 0 has run)
                rec[0] = hit ? vmax : 0;
                rec[1] = hit ? row0 + p + 1 : 0;          // half-open ends
                rec[2] = hit ? col_t - win_lane + 1 : 0;
            }
        }
        const int last_row = Rp[half] - 1 - row0;         // row Rp - 1, counted from the strip's first
        if (last_row >= 0 && last_row < geo::kRows && last_row / K == l) {
            int gs = 0, gt = 0;
#pragma unroll
            for (int q = 0; q < K; ++q) {
                if (q == last_row % K) {
                    gs = rb[half][q];
                    gt = fc[half][q];
                }
            }
            rec[3] = gs;
            rec[4] = gt - l + 1;                          // step -> column, half-open: the border column is 0
        }
    }
}

#ifdef VALIGN_TU_EXTEND      // not templates: defined once, in engine_extend.hip
// Trimmed lengths of a chunk's pairs, one wave per pair: lens[2 * pair] = Rp, lens[2 * pair + 1] = Fp -- 1 + the position of the
// last ACGT byte (either case), 0 where there is none.
__global__ void __launch_bounds__(64)
extend_wide_lengths_kernel(const uint8_t *reads, const uint8_t *refs, long long n, int R, int F, int *lens) {
    const long long pair = blockIdx.x;
    if (pair >= n) return;
    const int lane = threadIdx.x;
    int rlen = 0, flen = 0;
    for (int i = lane; i < R; i += kWave) {
        const int c = base_class(reads[pair * R + i]);
        if (c >= 1 && c <= 4) rlen = i + 1;
    }
    for (int jj = lane; jj < F; jj += kWave) {
        const int c = base_class(refs[pair * F + jj]);
        if (c >= 1 && c <= 4) flen = jj + 1;
    }
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const int other_r = __shfl_xor(rlen, d, kWave), other_f = __shfl_xor(flen, d, kWave);
        rlen = other_r > rlen ? other_r : rlen;
        flen = other_f > flen ? other_f : flen;
    }
    if (lane == 0) {
        lens[2 * pair] = rlen;
        lens[2 * pair + 1] = flen;
    }
}

// The merged partial records -> the call's records; a read without an ACGT byte is five zeros (no strip wrote its read-end score)
// band_half < 0: the unbanded sweep.  drop_rows (null: the key extend_zdrop is off): the read end of a pair that dropped is unreached.
__global__ void __launch_bounds__(256)
extend_wide_records_kernel(const int *partial, const int *lens, ExtendRec *extend, long long n, int band_half, const int *drop_rows) {
    const long long pair = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pair >= n) return;
    const int *rec = partial + kExtendWideRecDwords * pair;
    const bool empty = lens[2 * pair] == 0;
    ExtendRec r;
    r.score = empty ? 0 : rec[0];
    r.read_end = empty ? 0 : rec[1];
    r.ref_end = empty ? 0 : rec[2];
    // band_half >= 0 (the banded sweep): an unreached read end in closed form -- the strip that holds row Rp - 1 may have
    // returned before it wrote the pair
    const bool unreached = (band_half >= 0 && extend_band_unreached(lens[2 * pair], lens[2 * pair + 1], band_half)) ||
                           (drop_rows && extend_zdrop_unreached(drop_rows[pair], lens[2 * pair]));
    r.gscore = empty ? 0 : (unreached ? VALIGN_HIP_EXTEND_UNREACHED : rec[3]);
    r.gref_end = empty || unreached ? 0 : rec[4];
    extend[pair] = r;
}
#endif

}  // namespace valign
