// extend_zdrop.h -- the Z-drop of extension scores and alignments (key extend_zdrop; include/valign_hip.h has the definition,
// tests/extend_zdrop_ref.py restates it): what a call under the key is -- refused, or the int32 strip sweep with or without a band
// -- and the row-wise drop rule itself: the step of the running best, the associative combine of the prefix arg-max the sweep's
// epilogue scans with, and when a strip is skipped.  Integers in, integers out; no HIP: one definition for the engine, the kernel
// (extend_wide_kernels.hip.h, ZDROP) and the CPU check (tests/extend_zdrop_rules_check.cpp).  Below them, for the key
// extend_zdrop_rows: the rule's lane form for the int16 register sweep (extend_kernels.hip.h / extend_align_kernels.hip.h, ZDROP) and
// the two choices that wrap the older ones (tests/extend_zdrop_rows_rules_check.cpp).
//
// The rule is BWA's ksw_extend one with this library's rows as read positions: per row the maximum m_i over the present candidates
// and its first column c_i; the running best (M, Mi, Mj) starts at the anchor (0, -1, -1) and moves to a row only with a strictly
// larger maximum; a row that does not move it DROPS iff M - m_i - pen > Z, pen the price of the diagonal offset between the row's
// maximum and the running best at the extension score of the direction.  No floor at zero, no shrinking of the row range.
//
// RANGE (int32 throughout): under extend_int32_ok / extend_band_int32_ok every cell lies in [-2^28, 2^28], so M - m_i lies in
// [0, 2^29]; |di - dj| <= R + F <= 32767 and a price is at most 32768, so 0 <= pen < 2^30; M - m_i - pen lies in (-2^30, 2^29] and
// is compared with Z <= 2^30: nothing wraps.  Z >= 2^29 never drops.
#pragma once

#include "cell_rules.h"

namespace valign {

constexpr int kExtendZdropMax = 1 << 30;            // the largest Z the key takes
constexpr int kExtendZdropNone = 0x7FFFFFFF;        // T of a pair that has not dropped: a value no row has
constexpr const char *kExtendZdropKeyRange = "extend_zdrop must be in [0, 2^30]";
inline bool extend_zdrop_key_ok(long long Z) { return Z >= 0 && Z <= kExtendZdropMax; }
// the call runs the sweep's ZDROP instances, carries a drop row per pair and counts skipped waves
__host__ __device__ inline bool extend_zdrop_on(int Z) { return Z > 0; }

// The running best: value, row and column of the row-major first maximum so far.  The anchor is (0, -1, -1).
struct ExtendZdropBest {
    int m, i, j;
};
__host__ __device__ inline ExtendZdropBest extend_zdrop_anchor() { return ExtendZdropBest{0, -1, -1}; }
// ... as the partial record keeps it (score, read_end = Mi + 1, ref_end = Mj + 1; three zeros for the anchor) and back
__host__ __device__ inline ExtendZdropBest extend_zdrop_from_record(int score, int read_end, int ref_end) {
    return ExtendZdropBest{score, read_end - 1, ref_end - 1};
}

// The combine of the prefix arg-max: `a` covers earlier rows than `b`; a later row wins only with a strictly larger value.
// Associative, with "no row" (m = INT32_MIN) as its neutral element on the right.
__host__ __device__ inline ExtendZdropBest extend_zdrop_combine(const ExtendZdropBest &a, const ExtendZdropBest &b) { return b.m > a.m ? b : a; }
__host__ __device__ inline ExtendZdropBest extend_zdrop_no_row() { return ExtendZdropBest{(int)0x80000000, 0, 0}; }

// What a gap score (<= 0) costs per base of diagonal offset
__host__ __device__ inline int extend_zdrop_price(int gap_score) { return gap_score < 0 ? -gap_score : gap_score; }

// One row of the rule: row i with maximum m at column c (the border column is -1).  Moves `best` to the row where m is strictly
// larger; otherwise answers whether the row drops under Z.  price_ref: |ext_ref| (linear gaps: |gap_ref|), price_read likewise.
__host__ __device__ inline bool extend_zdrop_step(ExtendZdropBest &best, int i, int m, int c, int Z, int price_ref, int price_read) {
    if (m > best.m) {
        best = ExtendZdropBest{m, i, c};
        return false;
    }
    const int di = i - best.i, dj = c - best.j;
    const int pen = di > dj ? (di - dj) * price_ref : (dj - di) * price_read;
    return best.m - m - pen > Z;                // (RANGE, above: inside int32)
}

// A strip > 0 (rows [512 strip, 512 strip + 512)) is skipped by a wave whose two pairs both dropped ABOVE it.  A drop at the strip's
// first row is not known before the strip has run.  Strip 0 always runs: it starts the records and the drop rows.
__host__ __device__ inline bool extend_zdrop_strip_skipped(int strip, int T0, int T1) {
    const int row0 = strip * kExtendBandStripRows;
    return strip > 0 && T0 < row0 && T1 < row0;
}
// The read end of a pair that dropped is unreached: the rows from T on count for nothing
__host__ __device__ inline bool extend_zdrop_unreached(int T, int Rp) { return T < Rp; }

// ---- what a call under the key is ----
constexpr const char *kExtendZdropNoInt16 = "extend_zdrop: Z-dropped extension scores run on int32 cells; score_width = 16 (int16 or refuse) is refused";
constexpr const char *kExtendZdropRange = "extend_zdrop: shape x scoring can leave the range the int32 cells keep below their borders' sentinel";
constexpr const char *kExtendZdropAlign = "extend_zdrop: Z-dropped extension alignments run on the banded route only (band_width > 0 with extend_band = 1 and "
                                          "extend_band_align = 1); a band of 2 * max(read_length, ref_length) is the unbanded alignment";

// Extension scores.  Z == 0: exactly extend_choice.  Z > 0: the mode bit and traceback_policy = 1 are refused first, with their
// texts; under a band the answer is extend_choice's (Band under extend_band = 1, with its refusals; the band's refusal without the
// key); without a band the route is Wide whatever extend_wide, the read length and score_width 0 / 32 say -- the int16 register
// sweep has no Z-drop form -- refused for score_width = 16 and where extend_int32_ok fails.
inline PlacedChoice extend_zdrop_choice(const RuleInputs &in, int alg, const PlacedFacts &f, int G, int K, int Z) {
    const PlacedChoice plain = extend_choice(in, alg, f, G, K);
    if (!extend_zdrop_on(Z) || alg != kAlgSW || in.sse_policy || f.band_width > 0) return plain;
    PlacedChoice c;
    if (f.score_width == 16)
        c.reason = kExtendZdropNoInt16;
    else if (!extend_int32_ok(in))
        c.reason = kExtendZdropRange;
    else
        c.route = PlacedRoute::Wide;
    return c;
}

// Extension alignments.  Z == 0: exactly extend_align_choice.  Z > 0: the banded route (extend_band = 1, extend_band_align = 1,
// band_width > 0) answers as without the key -- Band, or its refusals; everything else the mode bit or the policy does not refuse
// first is refused with one text.
inline ExtendAlignChoice extend_zdrop_align_choice(const RuleInputs &in, int alg, const PlacedFacts &f, int G, int K, int Z) {
    const ExtendAlignChoice plain = extend_align_choice(in, alg, f, G, K);
    if (!extend_zdrop_on(Z) || alg != kAlgSW || in.sse_policy) return plain;
    if (f.band_width > 0 && f.extend_band && f.extend_band_align) return plain;
    ExtendAlignChoice c;
    c.reason = kExtendZdropAlign;
    return c;
}

// ---- key extend_zdrop_rows: the rule on the int16 register sweep (score_extend_kernel / align_extend_fill_kernel, ZDROP) ----
// The register sweep ends with every row's maximum and first column in registers -- a group of G lanes, lane l holding rows
// l K .. l K + K - 1 of one pair -- so the drop is decided in the epilogue; no cell, pointer or step changes.
//
// THE LANE FORM.  1. each lane combines its rows below Rp (extend_zdrop_combine, strict); 2. an exclusive prefix over the group's
// lanes, seeded with the anchor; 3. each lane replays its rows from its prefix (extend_zdrop_replay_lane); 4. T is the minimum
// of the lanes' answers.  Why the minimum is the serial rule's T: the prefix of a lane is the arg-max over ALL rows above the
// lane's first, which is the serial running best there only if no row above dropped.  So every lane whose rows lie at or above
// the true first drop holds the serial running best and replays the serial loop: the lane of the true T answers T, the lanes above
// it answer nothing.  A lane below the true T may hold a prefix the serial loop never reached, but whatever it answers is one of
// its own rows, all greater than T.  The record is the replay of lane T / K stopped at T; where nothing drops (T == Rp) the
// inclusive best of the last lane with a row below Rp.
//
// RANGE.  The register route runs only where every cell stays inside int16 (extend_int16_ok), so after sign-extension M - m lies
// in [0, 65535]; pen < 2^30 by the argument above; M - m - pen lies in (-2^30, 2^16) and is compared with Z <= 2^30 in int32.
constexpr int kExtendZdropUnreached = (int)0x80000000;        // gscore of a dropped pair: VALIGN_HIP_EXTEND_UNREACHED (include/valign_hip.h)
constexpr const char *kExtendZdropRowsKeyRange = "extend_zdrop_rows must be 0 or 1";
inline bool extend_zdrop_rows_key_ok(long long on) { return on == 0 || on == 1; }

struct ExtendZdropLane {
    int T;                      // the lane's first dropping row below Rp and below the stop row, kExtendZdropNone where none drops
    ExtendZdropBest best;       // the running best as it stands at min(T, stop_row): no row from there on has moved it
};
// One lane's replay: its K row entries (m[q], c[q]) are rows first_row + q; rows at or beyond Rp or stop_row count for nothing.
__host__ __device__ inline ExtendZdropLane extend_zdrop_replay_lane(const int *m, const int *c, int K, int first_row, int Rp, int stop_row,
                                                                    const ExtendZdropBest &prefix, int Z, int price_ref, int price_read) {
    ExtendZdropLane out{kExtendZdropNone, prefix};
    for (int q = 0; q < K; ++q) {
        const int row = first_row + q;
        if (out.T == kExtendZdropNone && row < Rp && row < stop_row && extend_zdrop_step(out.best, row, m[q], c[q], Z, price_ref, price_read)) out.T = row;
    }
    return out;
}
// ... and step 1 of the lane form: the combine of the lane's rows below Rp ("no row" where it has none)
__host__ __device__ inline ExtendZdropBest extend_zdrop_lane_best(const int *m, const int *c, int K, int first_row, int Rp) {
    ExtendZdropBest mine = extend_zdrop_no_row();
    for (int q = 0; q < K; ++q)
        if (first_row + q < Rp) mine = extend_zdrop_combine(mine, ExtendZdropBest{m[q], first_row + q, c[q]});
    return mine;
}
// The lane whose replay is the record: T / K of a dropped pair, the last lane with a row below Rp otherwise (Rp > 0)
__host__ __device__ inline int extend_zdrop_record_lane(int T, int Rp, int K) { return (T < Rp ? T : Rp - 1) / K; }

constexpr const char *kExtendZdropRowsAlign = "extend_zdrop: the int32 route of unbanded extension alignments has no Z-drop form (extend_zdrop_rows = 1 runs Z-dropped "
                                              "unbanded extension alignments on the int16 register sweep only; this call's shape, scoring or keys leave it)";

// Extension scores under the key.  Read only where Z > 0 and no band is set: where plain extend_choice answers the register route
// the call is Rows (score_width = 16 included); everything else is extend_zdrop_choice's answer.  rows_key = false, Z == 0 or a
// band: exactly extend_zdrop_choice.
inline PlacedChoice extend_zdrop_rows_choice(const RuleInputs &in, int alg, const PlacedFacts &f, int G, int K, int Z, bool rows_key) {
    if (rows_key && extend_zdrop_on(Z) && f.band_width == 0) {
        const PlacedChoice plain = extend_choice(in, alg, f, G, K);
        if (plain.route == PlacedRoute::Rows) return plain;
    }
    return extend_zdrop_choice(in, alg, f, G, K, Z);
}
// ... does the call run the register sweep's ZDROP instances?
inline bool extend_zdrop_rows_runs(const PlacedChoice &c, const PlacedFacts &f, int Z, bool rows_key) {
    return rows_key && extend_zdrop_on(Z) && f.band_width == 0 && c.route == PlacedRoute::Rows;
}

// Extension alignments under the key.  Read only where Z > 0 and no band is set: Rows wherever plain extend_align_choice answers
// the register route; every other unbanded call the mode bit or the policy does not refuse first is refused with
// kExtendZdropRowsAlign.  rows_key = false, Z == 0 or a band: exactly extend_zdrop_align_choice.
inline ExtendAlignChoice extend_zdrop_rows_align_choice(const RuleInputs &in, int alg, const PlacedFacts &f, int G, int K, int Z, bool rows_key) {
    const ExtendAlignChoice today = extend_zdrop_align_choice(in, alg, f, G, K, Z);
    if (!rows_key || !extend_zdrop_on(Z) || alg != kAlgSW || in.sse_policy || f.band_width > 0) return today;
    const ExtendAlignChoice plain = extend_align_choice(in, alg, f, G, K);
    if (plain.route == PlacedRoute::Rows) return plain;
    ExtendAlignChoice c;
    c.reason = kExtendZdropRowsAlign;
    return c;
}
inline bool extend_zdrop_rows_runs(const ExtendAlignChoice &c, const PlacedFacts &f, int Z, bool rows_key) {
    return rows_key && extend_zdrop_on(Z) && f.band_width == 0 && c.route == PlacedRoute::Rows;
}

}  // namespace valign
