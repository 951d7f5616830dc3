// ckpt_plan.h -- checkpointed traceback of long-read alignments (trace_checkpoints = 1, AlignRoute::StripCkpt) before its
// launches: what a pair-of-pairs holds in the scratch, how much of the batch the scratch takes at a time, and the order of the
// backward rounds.  Integers in, integers out; no HIP (tests/ckpt_plan_check.cpp exercises it on the CPU, as align_parts.h).
// The sizes are those of strip_plan.h -- the one plan of the strip path -- under the names this schedule gives them.
//
// The schedule (Engine::align_strips_device): the read is swept in S strips of 64 K rows.  The forward pass stores no
// pointers and keeps EVERY strip's bottom row -- S - 1 boundary-row sets (H; F beside it with affine gaps) instead of the two
// that ping-pong on the full-pointer path.  Then, for s = S - 1 down to 0, strip s is filled again with pointers into ONE
// strip-sized region (from checkpoint row s - 1, columns [0, c] only: c the walk's current column) and the walk crosses it,
// leaving its state -- row, column, cell value, output position, affine state -- for the next round.
#pragma once

#include <stddef.h>

#include <algorithm>
#include <vector>

#include "strip_plan.h"

namespace valign {

struct CkptPlan {
    int rows = 0;                   // rows per strip: 64 K
    int strips = 0;                 // S
    int pad_total = 0;              // padding rows above row 0, all in strip 0
    int blocks8 = 0;                // 8-step blocks per lane of one strip sweep
    int row_dwords = 0;             // dwords per boundary row (a multiple of 64)
    int row_sets = 0;               // boundary rows per checkpoint: H, and F with affine gaps
    // per pair-of-pairs (= one wave):
    size_t region_bytes = 0;        // the one pointer region every round reuses
    size_t row_bytes = 0;           // the S - 1 checkpoints
    size_t state_bytes = 0;         // the walk state of the two pairs
    size_t bytes_per_pp = 0;        // all of it
    size_t full_bytes = 0;          // what the full-pointer path holds instead: S regions
};

// The checkpointed strip plan (strip_plan.h) of unbanded int16 cells, and what the full-pointer path holds beside it
inline CkptPlan ckpt_plan(int R, int F, int K, bool affine) {
    const StripPlan s = strip_plan(R, F, K, StripMode{kAlgSW, affine, false, false, false, true}, kNoBand);
    return CkptPlan{s.rows,     s.strips,      s.pad_total,    s.blocks8,      s.row_dwords,
                    s.row_sets, s.strip_words * 4, s.row_bytes, s.state_bytes, s.bytes_per_pp, s.strip_words * 4 * s.strips};
}

// Pairs (an even number: whole waves) a scratch of at most `cap` bytes takes at a time -- at least one wave, at most the batch.
// The rule of the full-pointer strips, applied to whatever a pair-of-pairs holds there.
inline long long strip_chunk_pairs(size_t cap, size_t bytes_per_pp, long long n) {
    const long long chunk = std::max<long long>(2, (long long)(cap / bytes_per_pp) * 2);
    return std::min(chunk, (n + 1) / 2 * 2);
}

// The backward rounds: strip indices S - 1 .. 0.  Rounds go by strip and not by each pair's own progress, so that both pairs of
// a packed register are in the same strip in every round.
inline std::vector<int> ckpt_rounds(int strips) {
    std::vector<int> r;
    for (int s = strips - 1; s >= 0; --s) r.push_back(s);
    return r;
}

// The strip that holds read row i (padding rows lie above row 0, in strip 0; i = -1, "before the read", counts as strip 0)
// (constexpr: the kernels call it too)
constexpr int ckpt_strip_of_row(int i, int pad_total, int rows) { return i < 0 ? 0 : (i + pad_total) / rows; }

}  // namespace valign
