// extend_zdrop.h -- the Z-drop of extension scores and alignments (key extend_zdrop; include/valign_hip.h has the definition,
// tests/extend_zdrop_ref.py restates it): what a call under the key is -- refused, or the int32 strip sweep with or without a band
// -- and the row-wise drop rule itself: the step of the running best, the associative combine of the prefix arg-max the sweep's
// epilogue scans with, and when a strip is skipped.  Integers in, integers out; no HIP: one definition for the engine, the kernel
// (extend_wide_kernels.hip.h, ZDROP) and the CPU check (tests/extend_zdrop_rules_check.cpp).
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

}  // namespace valign
