// strip_plan.h -- the row-strip path of an alignment call (Engine::align_strips_device) before its launches: what the call is
// (StripMode), which kernel instances are compiled for it, how many rows a lane takes, what a pair-of-pairs holds in the scratch
// and where each piece lies.  Integers in, integers out; no HIP (tests/strip_plan_check.cpp exercises it on the CPU).
// The read is swept in S strips of 64 K rows, a launch each: a strip streams its pointers into a region of its own and hands its
// bottom row on through one of two boundary row sets that ping-pong; the checkpointed traceback (ckpt_plan.h) keeps ONE region,
// a row set per strip but the last, and the walk states of the pairs.
#pragma once

#include <stddef.h>

#include <algorithm>

#include "band_window.h"
#include "cell_rules.h"

namespace valign {

constexpr int kWalkStateBytes = 24;         // sizeof(WalkState) (trace_kernels.hip.h), per pair
constexpr int kStripKs[] = {16, 12, 8};     // rows per lane of the strip kernels, in the order the rows-per-lane rule tries them
constexpr BandShape kNoBand{-1, 1, 1, 0};

// What a strip call is.  strip_mode() is the only place the route is decoded.
// affine: a second code stream and F rows beside the H rows; sse: traceback_policy = 1; wide: int32 cells, one pair per
// register; band: the strips sweep their rows' band windows only; ckpt: checkpointed traceback
struct StripMode {
    int alg = kAlgSW;
    bool affine = false, sse = false, wide = false, band = false, ckpt = false;
};

inline StripMode strip_mode(AlignRoute route, const RuleInputs &in, int alg) {
    // (align_route returns the strip routes before it reaches this refusal of the register side)
    if (in.sse_policy && in.sc.affine)
        throw std::runtime_error("traceback_policy = 1 (SSE/AVX tie-breaks) exists for the linear gap model only");
    return StripMode{alg, in.sc.affine, in.sse_policy, route == AlignRoute::StripWide || route == AlignRoute::StripWideBand,
                     route == AlignRoute::StripBand || route == AlignRoute::StripWideBand, route == AlignRoute::StripCkpt};
}

// The kernel instances that are compiled (engine_align.hip instantiates exactly these).  int16 cells, unbanded: plain, affine,
// SSE tie-breaks and the checkpointed passes at every K; int32 cells: every mode at 8 rows per lane, at 16 / 12 the NW variant
// with linear gaps and default tie-breaks (the reference's model: long reads whose column-0 border leaves int16); bands: int16
// cells at 16 and 8 rows per lane, int32 cells at 8.
constexpr bool strip_instance_exists(int K, const StripMode &m) {
    if (K != 16 && K != 12 && K != 8) return false;
    if ((m.sse && (m.affine || m.band)) || (m.ckpt && (m.sse || m.band || m.wide))) return false;
    if (m.band) return m.wide ? K == 8 : K != 12;
    if (m.wide) return K == 8 || (m.alg == kAlgNW && !m.affine && !m.sse);
    return true;
}

// 16 rows per lane unless fewer leave less padding: 1 024-row strips cost 136 ms where 768-row strips cost 152 and 512-row
// strips 156 (10 kbp x 10 kbp, 4 096 pairs; 24 and 32 rows per lane -- 218 / 221 ms, two waves per SIMD by their
// registers -- are gone).  forced_k (debug switch strip_k): that K or none.  0: no instance serves the mode.
inline int strip_rows_per_lane(int R, const StripMode &m, int forced_k) {
    int best = 0;
    double best_cost = 0.0;
    for (int K : kStripKs) {
        if (!strip_instance_exists(K, m) || (forced_k && K != forced_k)) continue;
        const int rows = 64 * K;
        const double cost = (double)((R + rows - 1) / rows) * rows * (K == 16 ? 1.0 : (K == 12 ? 1.115 : 1.147));
        if (!best || cost < best_cost) {
            best = K;
            best_cost = cost;
        }
    }
    return best;
}

// The block band of a banded call on a read of R rows
inline BandShape strip_band_shape(int R, int band_width, int block_rows, int col_align) {
    return BandShape{band_width / 2, block_rows, col_align, (R + block_rows - 1) / block_rows * block_rows - R};
}

struct StripPlan {
    int rows = 0, strips = 0;       // rows per strip: 64 K; S
    int pad_total = 0;              // padding rows above row 0, all in strip 0
    int max_cols = 0;               // columns of the widest strip window (unbanded: F); it sizes every strip's region
    int blocks8 = 0;                // 8-step blocks per lane of one strip sweep
    int row_dwords = 0;             // dwords per boundary row (a multiple of 64)
    int row_sets = 0;               // boundary rows per set: H, and F beside it (affine); int32 cells: those per pair
    bool ckpt = false;              // checkpointed traceback
    int regions = 0, set_slots = 0; // pointer regions / row sets held at a time: S / the 2 that ping-pong, checkpointed 1 / S - 1
    BandShape band = kNoBand;
    size_t strip_words = 0;         // per pair-of-pairs (= one wave) from here on: dwords of one strip's pointer region
    size_t row_bytes = 0;           // the row sets
    size_t state_bytes = 0;         // checkpointed: the walk state of the two pairs
    size_t bytes_per_pp = 0;        // all of it
    long long ptr_bytes_per_pair = 0, ckpt_bytes_per_pair = 0;      // describe(): align_ptr_bytes_per_pair, align_ckpt_bytes_per_pair

    // The scratch of a chunk, in dwords from its start.  waves: pairs-of-pairs the scratch is sized for; cnt_waves: those of the
    // chunk that runs (the last one may be shorter: its regions lie closer together)
    size_t region_stride(long long cnt_waves) const { return (size_t)cnt_waves * strip_words; }
    size_t region_at(long long cnt_waves, int s) const { return ckpt ? 0 : (size_t)s * region_stride(cnt_waves); }
    size_t boundary_at(long long waves) const { return (size_t)waves * strip_words * regions; }
    // one boundary row of every wave; the F rows of a set lie this far behind its H rows
    size_t f_rows_at(long long waves) const { return (size_t)waves * row_dwords; }
    // the row set strip s writes: the two that ping-pong -- or, checkpointed, its own (the last strip writes none); the one it
    // reads: what strip s - 1 wrote (strip 0 reads none)
    size_t bottom_at(long long waves, int s) const {
        const int slot = ckpt ? std::min(s, std::max(strips - 2, 0)) : (s & 1);
        return boundary_at(waves) + (size_t)slot * row_sets * f_rows_at(waves);
    }
    size_t top_at(long long waves, int s) const { return bottom_at(waves, s > 0 ? s - 1 : 0); }
    size_t walk_at(long long waves) const { return boundary_at(waves) + (size_t)set_slots * row_sets * f_rows_at(waves); }      // (checkpointed)
};

inline StripPlan strip_plan(int R, int F, int K, const StripMode &m, const BandShape &band) {
    StripPlan p;
    p.rows = 64 * K;
    p.strips = std::max(1, (R + p.rows - 1) / p.rows);
    p.pad_total = p.strips * p.rows - R;
    p.band = m.band ? band : kNoBand;
    for (int s = 0; s < p.strips; ++s) {        // (no band: every window is [0, F))
        int c_lo, cols;
        band_rows_window(p.band, s * p.rows - p.pad_total, (s + 1) * p.rows - p.pad_total - 1, R, F, c_lo, cols);
        p.max_cols = std::max(p.max_cols, cols);
    }
    p.blocks8 = (p.max_cols + 63 + 7) / 8;
    p.row_dwords = ((F + 71) / 64 + 2) * 64;
    p.row_sets = (m.affine ? 2 : 1) * (m.wide ? 2 : 1);
    p.ckpt = m.ckpt;
    p.regions = m.ckpt ? 1 : p.strips;
    p.set_slots = m.ckpt ? p.strips - 1 : 2;
    p.strip_words = (size_t)p.blocks8 * 64 * K * (m.affine ? 2 : 1);
    p.row_bytes = (size_t)p.set_slots * p.row_sets * p.row_dwords * 4;
    p.state_bytes = m.ckpt ? (size_t)2 * kWalkStateBytes : 0;
    p.bytes_per_pp = p.strip_words * 4 * p.regions + p.row_bytes + p.state_bytes;
    p.ptr_bytes_per_pair = (long long)(p.strip_words * 4 * p.regions / 2);
    p.ckpt_bytes_per_pair = m.ckpt ? (long long)((p.row_bytes + p.state_bytes) / 2) : 0;
    return p;
}

// What the scratch may take of the device: half of the free HBM (`free_bytes`: free bytes plus the scratch held already), at
// least 256 MiB, at most 128 GiB, then the configured cap.  (The pointer stream of a 10 kbp x 10 kbp pair-of-pairs is 50 MB:
// what fits the scratch is what runs side by side -- 24 GB, the bound until round 4, kept 480 waves on 1 024 SIMDs.)
inline size_t strip_scratch_cap(size_t free_bytes, long long cap_mb) {
    const size_t cap = std::min<size_t>(128ull << 30, std::max<size_t>(free_bytes / 2, 256ull << 20));
    return cap_mb > 0 ? std::min<size_t>(cap, (size_t)cap_mb << 20) : cap;
}

}  // namespace valign
