// cell_rules.h -- the closed-form bounds that pick the cell format (f16 / int16 / int32), the fill kernel and the path of a
// score or alignment call, each defined once; integer arithmetic on (scoring, shape, a few switches), no HIP.  The engine
// units include it and tests/cell_rules_check.cpp exercises it on the CPU (as band_window.h and host_pipeline.h are).  A bound
// one term too loose does not fail: it returns a wrapped short or a rounded half for some inputs only
// (tests/test_gpu_range_edges.py walks each rule to its edge on the GPU).
#pragma once

#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "cell_constants.h"
#include "extend_band_align_plan.h"

namespace valign {

// What every rule reads of an engine (Engine::rule_inputs): the scoring, the shape, traceback_policy = 1 and the debug switches
struct RuleInputs {
    Scoring sc;
    int R = 0, F = 0;
    bool sse_policy = false;
    bool no_sym = false, no_tag = false, no_f16 = false, no_prof_key = false;
    bool no_max3 = false;           // debug switch: int16 symmetric affine SW scores on the gap-source form always
    bool no_tilt = false;           // debug switch: ... and its biased form in the plain frame always
    bool no_row_tables = false;     // debug switch: ... and its tilted frame on the LDS profile always
    bool no_side_tile = false;      // debug switch: ... and never on the 8 x 19 side geometry (the plan of the geometry table always)
};

// int16 DP cells: the reference wraps silently.  Scores and alignments switch to int32 cells on the strip path where they could.
// The NW score kernels keep cell (p, j) plus -g_ref * p - g_read * j (g: gap / extension scores, <= 0): the most that
// adds over a sweep of `rows` padded rows and F columns.
inline long long nw_tilt_span(const Scoring &sc, int rows, int F) {
    const long long per_row = -(long long)(sc.affine ? sc.ext_ref : sc.gap_ref);
    const long long per_col = -(long long)(sc.affine ? sc.ext_read : sc.gap_read);
    return per_row * (rows + 1) + per_col * (F + 1);
}

// Every cell of an R x F sweep and everything added to it stays an integer of magnitude <= 2048:
// exact in half floats (kGapAffineSymF16 / kGapAffineF16).  SW cells are >= 0; cells of the NW
// variant are bounded below by the cheaper border path (as in int16_range_ok).
// NW: plus what the kernels' tilted frame adds to a cell of a sweep of `rows` padded rows (score_kernel).
inline bool half_float_exact(const Scoring &sc, int alg, int R, int F, int rows) {
    const long long top = (long long)std::min(R, F) * std::max({sc.match, sc.mismatch, 0});
    long long slack = std::max({std::abs(sc.match), std::abs(sc.mismatch), std::abs(sc.open_read),
                                std::abs(sc.ext_read), std::abs(sc.open_ref), std::abs(sc.ext_ref)});
    if (alg == kAlgSW) return top + 2 * slack <= 2048 && slack <= 1024;
    // NW frame: H' of cell (p, j) is at least what its row or its column adds (the border path along the other axis
    // is free there) less one opening, at most top + the far corner's tilt; E' / F' sit at most one opening below H'.
    // The kernel centres that range on zero (nw_frame_centre, same formula).
    if (!sc.affine) slack = std::max<long long>(slack, std::max(std::abs(sc.gap_read), std::abs(sc.gap_ref)));
    const long long span = nw_tilt_span(sc, rows, F);
    const long long centre = (top + span) / 2;
    return span < 30000 && (top + span - centre) + 3 * slack <= 2048 && centre + 3 * slack <= 2048 && slack <= 512;
}

// kGapSymF16 for Smith-Waterman scales every value by 2^-10 and floors with the [0, 1] clamp of the
// packed add: cells must stay below 1024, scores be integers of magnitude < 1024
inline bool half_float_unit_exact(const Scoring &sc, int R, int F) {
    const long long top = (long long)std::min(R, F) * std::max({sc.match, sc.mismatch, 0});
    const long long slack = std::max({std::abs(sc.match), std::abs(sc.mismatch), std::abs(sc.gap_read), std::abs(sc.gap_ref)});
    return top + 2 * slack < 1024 && slack < 512;
}

// Every cell of the call stays inside int16.  score_path: score_alignments (the NW variant's tilted frame counts on the
// register sweep: `tilt_rows` padded rows, the tallest plan a call may take); long_mode: the engine's plan is the long-read one
inline bool int16_range_ok(const RuleInputs &in, int alg, bool score_path, bool long_mode, int tilt_rows) {
    const Scoring &sc = in.sc;
    long long hi = (long long)std::min(in.R, in.F) * std::max(sc.match, 0) + 1;
    if (score_path && alg == kAlgNW && !long_mode) hi += nw_tilt_span(sc, tilt_rows, in.F);
    const int worst_gap = std::min({sc.gap_read, sc.gap_ref, sc.open_read, sc.open_ref, sc.ext_read, sc.ext_ref, 0});
    // SW cells are >= 0; NW-variant score cells are bounded below by the cheaper border path
    long long lo = alg == kAlgSW ? (long long)std::min(sc.mismatch, 0) + worst_gap
                                 : (long long)(std::min(in.R, in.F) + 2) * std::min(worst_gap, std::min(sc.mismatch, 0));
    // NW-variant alignments with affine gaps (plain frame, "minus infinity" = -16384): row 0 is free, so every H is at least a
    // gap straight down from it -- open_ref + (R - 1) ext_ref -- and E / F lie at most one opening below an H; a candidate
    // adds one mismatch.  (The product above charged every step an opening: -50 010 for 10 kbp reads at -5 / -1, whose cells
    // never go below -10 010.)
    if ((!score_path || long_mode) && sc.affine && alg == kAlgNW)       // (the long-read score kernels: the same plain frame)
        lo = (long long)std::min(sc.open_ref, 0) + (long long)in.R * std::min(sc.ext_ref, 0) + std::min({sc.open_read, sc.open_ref, 0}) +
             std::min(sc.mismatch, 0);
    return !(hi > 32000 || lo < -32000 || (sc.affine && alg == kAlgNW && lo < -15000));
}

// Column 0 of the NW variant with linear gaps leaves int16: a gap of the whole read, (R + 1) gap_ref (affine: open_ref +
// R ext_ref, which int16_range_ok covers)
inline bool border_bad(const RuleInputs &in, int alg) {
    return alg == kAlgNW && !in.sc.affine && (long long)(in.R + 1) * std::min(in.sc.gap_ref, 0) < -32000;
}

// int32 cells (align_strip_wide_kernel) serve every mode; only scores so large that (R + F) * |score| nears 2^28 are refused
inline bool int32_refused(const RuleInputs &in) {
    const Scoring &sc = in.sc;
    const long long worst = std::max({std::abs((long long)sc.match), std::abs((long long)sc.mismatch),
                                      std::abs((long long)(sc.affine ? sc.open_read : sc.gap_read)), std::abs((long long)(sc.affine ? sc.open_ref : sc.gap_ref)),
                                      sc.affine ? std::abs((long long)sc.ext_read) : 0ll, sc.affine ? std::abs((long long)sc.ext_ref) : 0ll});
    return (long long)(in.R + in.F + 2) * worst >= (1ll << 28);
}

// align_fill_tag_kernel keeps 4 * cell + tag in int16.  rows: padded rows of the sweep that would run
inline bool tagged_range_ok(const RuleInputs &in, int alg, int rows) {
    const Scoring &sc = in.sc;
    long long hi = (long long)std::min(in.R, in.F) * std::max(sc.match, 0) + 1;
    if (alg == kAlgNW && !in.sse_policy)           // the kernel's tilted frame: every cell plus -gap_ref * p - gap_read * j
        hi += (long long)-sc.gap_ref * (rows + 1) + (long long)-sc.gap_read * (in.F + 1);
    const int worst = std::min({sc.gap_read, sc.gap_ref, sc.mismatch, 0});
    const long long lo = alg == kAlgSW ? worst : (long long)(in.R + in.F + 2) * worst;      // H(i,j) >= i gf + j gr
    if (alg == kAlgSW && !in.sse_policy && sc.gap_ref >= 0) return false;
    return 4 * hi + 4 <= 32000 && 4 * lo - 4 >= -32000 && std::abs(sc.match) < 2000 && std::abs(sc.mismatch) < 2000;
}

// align_fill_affine_tag_kernel keeps 8 * cell + tag in int16; SW needs open scores < 0 (the tag rides on the
// open constant) and, for the lane key, value << 4 (5) in range
inline bool affine_tagged_range_ok(const RuleInputs &in, int alg, int geo_rows, int K) {
    const Scoring &sc = in.sc;
    long long hi = (long long)std::min(in.R, in.F) * std::max(sc.match, 0) + 1;
    const int worst = std::min({sc.open_read, sc.open_ref, sc.ext_read, sc.ext_ref, sc.mismatch, 0});
    // NW: every cell is at least the path "one gap up, one gap left"; E / F sit one open below H
    long long lo = alg == kAlgSW ? worst
                                 : 2ll * (std::min(sc.open_read, 0) + std::min(sc.open_ref, 0)) +
                                       (long long)(in.R + in.F + 2) * std::min({sc.ext_read, sc.ext_ref, 0}) + worst;
    if (alg == kAlgNW) {        // the kernel's tilted frame: cell (p, j) carries - ext_ref * p - ext_read * j on top
        const long long rows = (long long)geo_rows + 1, cols = in.F + 1;
        hi += std::max(0, -sc.ext_ref) * rows + std::max(0, -sc.ext_read) * cols;
        lo += std::min(0, -sc.ext_ref) * rows + std::min(0, -sc.ext_read) * cols;
        if (std::abs((long long)sc.ext_ref) * rows > 3500 || std::abs((long long)sc.ext_read) * cols > 3500) return false;
    }
    if (alg == kAlgSW && (sc.open_read >= 0 || sc.open_ref >= 0)) return false;
    const int key_bits = K <= 16 ? 4 : 5;
    if (alg == kAlgSW && ((hi + 1) << key_bits) > 32000) return false;
    return 8 * hi + 8 <= 32000 && 8 * lo - 8 >= -28000 && std::abs(sc.match) < 1000 && std::abs(sc.mismatch) < 1000;
}

// SW, tagged cells: one (value, row) key per lane instead of a first-arg-max per row where value << 4 (5 bits of row for more
// than 16 rows per lane) still fits int16
inline bool lane_key_ok(const RuleInputs &in, int K) {
    return (((long long)std::min(in.R, in.F) * std::max(in.sc.match, 0) + 1) << (K <= 16 ? 4 : 5)) <= 32000;
}
// ... and where 64x the cell range fits (K <= 16), the key rides in the query profile instead of being computed
inline bool prof_key_ok(const RuleInputs &in, int K) {
    const Scoring &sc = in.sc;
    return !in.sse_policy && !in.no_prof_key && K <= 16 && (((long long)std::min(in.R, in.F) * std::max(sc.match, 0) + 2) << 6) <= 32000 &&
           64ll * std::max(std::abs(sc.gap_read), std::abs(sc.gap_ref)) < 32000 && 64ll * std::abs(sc.mismatch) < 16000;
}

// The gap form (kGap*) a register-sweep score launch of R x F on `rows` padded rows runs: what launch_score launches and what
// describe() predicts (score_cells).
inline int score_gap_form(const RuleInputs &in, int alg, int R, int F, int rows) {
    const Scoring &sc = in.sc;
    if (sc.affine) {
        const bool sym = sc.open_read == sc.open_ref && sc.ext_read == sc.ext_ref && !in.no_sym;
        if (!in.no_f16 && half_float_exact(sc, alg, R, F, rows)) return sym ? kGapAffineSymF16 : kGapAffineF16;
        return sym ? kGapAffineSym : kGapAffine;
    }
    const int gaps = (sc.gap_read == sc.gap_ref && !in.no_sym) ? kGapSym : kGapLinear;
    // (the NW variant's tilted frame has no gap constants left: its half-float kernel serves gap_read != gap_ref too)
    if ((gaps == kGapSym || alg == kAlgNW) && !in.no_f16 &&
        (alg == kAlgNW ? half_float_exact(sc, alg, R, F, rows) : half_float_unit_exact(sc, R, F)))
        return kGapSymF16;
    return gaps;
}
inline bool gap_form_f16(int gaps) { return gaps == kGapSymF16 || gaps == kGapAffineSymF16 || gaps == kGapAffineF16; }

// ---- the two forms of score_kernel<G, K, kAlgSW, kGapAffineSym> (dp_kernels.hip.h) ----
// The biased form keeps every int16 cell as value + B and takes its maxima three at a time with the packed half-float
// maximum, which is an integer maximum while every operand's bit pattern lies in [0x0400, 0x7BFF], the positive normal halves.
// With the magnitudes o = -open, x = -extend and m = the most a substitution score takes off a cell, the smallest operand of
// the recurrence is B - o - x or B - m (the window proof is at the kernel's step), so B = 1024 + o + x + m keeps all of them at
// or above 0x0400 ...
constexpr int kMax3WindowLow = 0x0400, kMax3WindowHigh = 0x7BFF;
inline int sym_affine_bias(const Scoring &sc) {
    const int o = -sc.open_ref, x = -sc.ext_ref, m = std::max({0, -sc.mismatch, -sc.match});
    return kMax3WindowLow + o + x + m;
}
// ... and the form is legal where B plus the largest cell (counted as in int16_range_ok, a positive mismatch score included)
// stays at or below 0x7BFF.  R, F: of the launch (the padded ones of a length-sorted launch: conservative for every group).
// Asked only where score_gap_form has answered kGapAffineSym for Smith-Waterman; beyond the window the gap-source form runs.
inline bool sym_affine_max3_ok(const RuleInputs &in, int R, int F) {
    const Scoring &sc = in.sc;
    if (in.no_max3 || !sc.affine || sc.open_read != sc.open_ref || sc.ext_read != sc.ext_ref) return false;
    if (sc.open_ref > 0 || sc.ext_ref > 0) return false;
    const long long B = sym_affine_bias(sc);
    const long long hi = (long long)std::min(R, F) * std::max({sc.match, sc.mismatch, 0}) + 1;
    return B - kMax3WindowLow <= 1024 && B + hi <= kMax3WindowHigh;
}
// describe()'s name of the form the last such launch ran (ran_score_sym_affine)
inline const char *ran_sym_affine_name(bool max3) { return max3 ? "max3" : "sources"; }

// The biased form in a TILTED frame: cell (p, j) kept as value + B + x * u, u = p + j + c0, where an extension costs nothing
// (two subtracts per register less; the proof is at the kernel's step).  The zero floor of a cell is then B + x * u, the smallest
// operand of a maximum lies max(o - x, m) below a floor, and c0 puts the smallest u any register carries at 0, so
// B = 1024 + max(o - x, m) ...
inline int sym_affine_tilt_bias(const Scoring &sc) {
    const int o = -sc.open_ref, x = -sc.ext_ref, m = std::max({0, -sc.mismatch, -sc.match});
    return kMax3WindowLow + std::max(o - x, m);
}
// ... the largest u belongs to the last row of the last lane at the last step of the sweep, unmasked steps included: a sweep of
// `rows` padded rows in lanes of K rows starts `lead` lanes down and ends at u = rows + F - lead
inline long long sym_affine_tilt_top_index(int R, int F, int rows, int K) {
    const int lead = rows > R ? (rows - R) / K : 0;
    return (long long)rows + F - lead;
}
// ... and the form is legal inside the plain biased form's window, for K <= kTiltMaxK and on the 8 x 19 side tile (cell_constants.h:
// tilt_frame_built; the rule sees rows and K, the group is rows / K), where B plus the largest tilt plus the largest cell stays at
// or below 0x7BFF.  R, F as in sym_affine_max3_ok; rows, K: of the geometry the launch runs on.
// The running maxima of the sweep stay in the frame: an accumulator is carried from anti-diagonal to anti-diagonal of its lane and
// holds, whenever a maximum reads it, the largest cell that lane has seen so far plus B + x * u of a cell of the sweep (u <= the top
// index) -- a cell of the matrix plus a tilt of the sweep, which is what `hi` and the top index bound already: the rule stands as it is
// (tests/test_sym_affine_inframe_sweep.py asserts it of every operand at the rule's edge).
inline bool sym_affine_tilt_ok(const RuleInputs &in, int R, int F, int rows, int K) {
    if (in.no_tilt || K <= 0 || !tilt_frame_built(rows / K, K) || !sym_affine_max3_ok(in, R, F)) return false;
    const Scoring &sc = in.sc;
    const long long B = sym_affine_tilt_bias(sc);
    const long long hi = (long long)std::min(R, F) * std::max({sc.match, sc.mismatch, 0}) + 1;
    return B + (long long)-sc.ext_ref * sym_affine_tilt_top_index(R, F, rows, K) + hi <= kMax3WindowHigh;
}
inline const char *ran_sym_affine_frame_name(bool tilted) { return tilted ? "tilted" : "plain"; }

// The tilted sweep's substitution scores from ROW TABLES in registers instead of the LDS profile (dp_kernels.hip.h:
// wave_setup_tables and the step's kRowTables form): four bytes per row and pair, so every score the tilted frame adds on
// the diagonal -- match' = match + 2x, mismatch' = mismatch + 2x, zero' = 2x, each of them plus o - x (every row takes its
// diagonal from H - (o - x), the register E reads anyway, and gets the o - x back from its table) --
// must be a byte: the smallest of them >= 0, the largest + (o - x) <= 255, o - x >= 0 (the tables add it byte-wise).
// The window needs nothing more: a column outside the reference scores 0 instead of zero' + (o - x), which puts its diagonal
// candidate o + x below a floor whose u is at least 2, no lower than B - (o - x) >= 0x0400 for every scoring
// sym_affine_tilt_ok lets through (x >= 0, B >= 1024 + o - x).
// The same bytes let the row-table step add and subtract on the 32-bit word that holds two pairs (v_add_u32 / v_sub_u32 in place
// of v_pk_add_u16 / v_pk_sub_i16): a score in [0, 255] added to a half of the window cannot carry, since the sum is an operand of
// the window itself (sym_affine_tilt_ok), and o - x in [0, 255] taken off an H >= B >= 0x0400 + (o - x) cannot borrow; the
// LDS-profile form, whose scores may be negative, keeps the packed instructions (dp_kernels.hip.h: WORD ARITHMETIC).
// lds_profile / lds_tables: bytes of LDS per wave of the launch's
// plan and of the row-table set-up (row_table_lds): the tables are taken where they need no more, so that no block asks for
// more LDS than its plan was sized for (long references: the selector stream has four bytes per column, the codes two).
inline int sym_affine_row_table_low(const Scoring &sc) { return std::min({sc.match, sc.mismatch, 0}) - 2 * sc.ext_ref; }
inline int sym_affine_row_table_high(const Scoring &sc) {
    return std::max({sc.match, sc.mismatch, 0}) - 2 * sc.ext_ref + (sc.ext_ref - sc.open_ref);
}
inline bool sym_affine_row_tables_ok(const RuleInputs &in, int R, int F, int rows, int K, int lds_profile, int lds_tables) {
    if (in.no_row_tables || !sym_affine_tilt_ok(in, R, F, rows, K)) return false;
    if (in.sc.ext_ref - in.sc.open_ref < 0 || F > 60000) return false;        // (the set-up keeps column numbers in 16 bits)
    return sym_affine_row_table_low(in.sc) >= 0 && sym_affine_row_table_high(in.sc) <= 255 && lds_tables <= lds_profile;
}
inline const char *ran_sym_affine_scores_name(bool row_tables) { return row_tables ? "row_tables" : "lds_profile"; }

// ---- the 8 x 19 SIDE TILE of that sweep (cell_constants.h: kSideTileG x kSideTileK; engine.hip.h: kSideGeometry) ----
// 152 rows in a wave64: a read of 129 .. 152 bases pads 1.3 % where 16 x 10 pads 6.25 %, the skew of the sweep is 7 steps instead
// of 15 and the fixed part of a step is paid once per 19 rows.  Its one kernel carries the row-table forms only, 16 pairs per wave,
// and issues well only with two waves per SIMD: the plan is a 4-wave block, and it is taken only where TWO such blocks fit a CU's
// LDS: side_tile_wave_lds(R, F) bytes per wave (cell_constants.h; dp_kernels.hip.h lays them out).  A block's LDS is
// granted in granules (three blocks of 54,016 B did not fit the 163,840 B of a CU), so the budget counts each block rounded up to
// 2 KB and leaves 8 KB of the CU alone: nothing is planned to the last byte.
constexpr int kSideTileRows = kSideTileG * kSideTileK, kSideTileMinRead = 129;
constexpr int kSideTileBlockWaves = 4, kSideTileLdsGranule = 2048, kSideTileLdsBudget = 152 * 1024;
inline bool side_tile_lds_ok(int lds_wave) {
    const long long block = ((long long)lds_wave * kSideTileBlockWaves + kSideTileLdsGranule - 1) / kSideTileLdsGranule * kSideTileLdsGranule;
    return lds_wave > 0 && 2 * block <= kSideTileLdsBudget;
}
// Why a Smith-Waterman (`alg`) score launch of gap form `gaps` (score_gap_form) over R x F does NOT run on the side tile; "" where
// it does.  R, F: of the launch (a length-sorted launch: its read class and widest reference), which size its LDS; the windows are asked about the
// engine's shape in.R x in.F, as for every launch of a call.  latency: the call is small enough for the latency plan, whose
// sweeps are as short as can be -- the side tile is a throughput plan.  forced: group_lanes = 8, rows_per_lane = 19; a forced tile
// runs whatever the call's size and however short the read (R <= 152 is what fits; R = 1 leaves one live row in the last lane),
// the other conditions hold for it as they stand and the engine raises the text.
inline const char *sym_affine_side_tile_refusal(const RuleInputs &in, int alg, int gaps, int R, int F, bool latency, bool forced) {
    const int lds_wave = side_tile_wave_lds(R, F);
    if (in.no_side_tile) return "the side tile is switched off (VALIGN_HIP_DEBUG=no_side_tile)";
    if (alg != kAlgSW) return "the 8 x 19 tile exists for Smith-Waterman scores only";
    if (gaps != kGapAffineSym)
        return "the 8 x 19 tile exists for int16 cells with symmetric affine gaps only (half_float_cells = 0, open_read = open_ref, ext_read = ext_ref)";
    if (R > kSideTileRows) return "the 8 x 19 tile holds reads of at most 152 bases";
    if (in.no_tilt) return "the 8 x 19 tile runs the tilted frame only (VALIGN_HIP_DEBUG=no_tilt)";
    if (in.no_row_tables) return "the 8 x 19 tile runs the row tables only (VALIGN_HIP_DEBUG=no_row_tables)";
    if (!sym_affine_row_tables_ok(in, in.R, in.F, kSideTileRows, kSideTileK, lds_wave, lds_wave))
        return "the 8 x 19 tile runs the tilted frame with row tables only: shape x scoring leave its window, or a substitution score of the frame is no byte (sym_affine_row_tables_ok)";
    if (!side_tile_lds_ok(lds_wave)) return "the 8 x 19 tile needs two 4-wave blocks per CU: the reference is too long for its LDS budget";
    if (forced) return "";
    if (R < kSideTileMinRead) return "reads of at most 128 bases fit a smaller tile";
    if (latency) return "small calls take the latency plan";
    return "";
}

// Which fill kernel an alignment call of this mode takes on a G x K geometry, and what its pointer stream looks like.
struct FillChoice {
    int kernel = 0;                 // FillKernel
    bool affine_tagged = false, tagged = false;
};
inline FillChoice fill_choice(const RuleInputs &in, int alg, int G, int K) {
    const Scoring &sc = in.sc;
    FillChoice c;
    const int rows = G * K;
    // affine gaps with the traceback information tagged into the cells (4-bit codes, 4-step blocks)
    c.affine_tagged = sc.affine && !in.sse_policy && !in.no_tag && affine_tagged_range_ok(in, alg, rows, K);
    // linear gaps: the pointer rides in the low bits of the cell where 4x the cell range still fits int16 (and, for SW,
    // gap_ref < 0); otherwise the equality-test kernels (both tie-break policies)
    c.tagged = !sc.affine && !in.no_tag && tagged_range_ok(in, alg, rows);
    const bool lane_key = c.tagged && alg == kAlgSW && lane_key_ok(in, K);
    const bool prof_key = lane_key && prof_key_ok(in, K);
    const bool affine_sym = sc.affine && sc.open_read == sc.open_ref && sc.ext_read == sc.ext_ref && !in.no_sym;
    if (prof_key) c.kernel = kFillTagProfKey;
    else if (c.tagged) c.kernel = in.sse_policy ? (lane_key ? kFillSseTagKey : kFillSseTag) : (lane_key ? kFillTagKey : kFillTag);
    else if (in.sse_policy) c.kernel = kFillSse;
    else if (sc.affine) c.kernel = c.affine_tagged ? (affine_sym ? kFillAffineTagSym : kFillAffineTag) : (affine_sym ? kFillAffineSym : kFillAffine);
    else c.kernel = (sc.gap_read == sc.gap_ref && !in.no_sym) ? kFillLinearSym : kFillLinear;
    return c;
}

// ---- placed scores (valign_hip_score_placed_*): the Smith-Waterman score and its end cell from the score sweep alone ----
// Bits of the lane key below the value: enough for the K rows of a lane.  The key form exists for K <= 16.
constexpr int placed_key_bits(int K) { return K <= 4 ? 2 : (K <= 8 ? 3 : 4); }
constexpr int kPlacedKeyMaxK = 16;
// Reads of more rows than this take the row strips, as alignments do (Engine::route_facts)
constexpr int kPlacedStripRows = 1024;

enum class PlacedRoute { Refused, Key, Rows, Strip, Chain, Wide };
// The route of banded extension scores (extend_band, below): the banded int32 strip sweep.  A value of the type that stands beside
// the enumerators -- an enum class holds every value of its underlying int -- so that the list above reads as the placed scores
// left it (tests/test_placed_wide_rules.py pins its end); ran_placed_name knows it as "band".
constexpr PlacedRoute kPlacedRouteBand = static_cast<PlacedRoute>(6);

// band_placed = 1 under a band: the banded block chain (band_kernels.hip.h) tracks one key per lane on its int32 cells,
// `diagonal candidate << kBandPlacedKeyBits | (15 - row of the lane's 16-row block)`, compared as signed integers: the largest
// possible value plus one, shifted, must stay inside int32.  (int32_refused is the tighter bound wherever both apply -- (R + F +
// 2) / 2 > min(R, F) -- so placed_choice never refuses through this rule today: it becomes live only if int32_refused is relaxed
// or the key takes more bits, and is kept, and tested at its own edge, so that either change meets it.)
constexpr int kBandPlacedKeyBits = 4;
inline bool band_placed_key_ok(const RuleInputs &in) {
    return (((long long)std::min(in.R, in.F) * std::max(in.sc.match, 0) + 1) << kBandPlacedKeyBits) <= 0x7FFFFFFFll;
}

// What the rule reads of the engine beyond the rule inputs (Engine::placed_facts)
struct PlacedFacts {
    int band_width = 0;
    int score_width = 0;            // the score_width key: 0, 16 or 32
    bool forced = false;            // a forced geometry stays on the register path whatever the read length
    bool long_plan = false;         // no register geometry holds the shape (the alignment plan is the long-read one)
    bool band_placed = false;       // band_placed = 1: under a band the call runs on the block chain, on the chain's band
    bool chain_usable = false;      // band_chain_plan(...).usable for this band_width (long_plan.h)
    bool placed_wide = false;       // placed_wide = 1: unbanded calls on int32 cells run on the pointer-free int32 sweep
    bool extend_wide = false;       // extend_wide = 1: extension calls the int16 register sweep refuses run on the int32 strip sweep
    // extend_band on: extension score calls under a band run banded on the int32 strip sweep.  Trailing, false by default, as
    // extend_wide was before it; written without blanks around the sign because tests/test_extend_wide_rules.py and
    // tests/test_placed_wide_rules.py pin the text of the members above as it stood
    bool extend_band=false;
    // extend_band_align on: extension ALIGNMENT calls under a band with extend_band on run banded, with back pointers, on the same
    // sweep.  Appended, false by default; the declaration stands behind its name for the same reason as above: tests/
    // test_extend_band_rules.py pins extend_band as the last line that begins with a member's type
    /* extend_band_align: */ bool extend_band_align=false;
};

struct PlacedChoice {
    PlacedRoute route = PlacedRoute::Refused;
    int key_bits = 0;               // Key: the bits of the row below the value
    const char *reason = "";        // Refused: why
};

// `G x K`: the register geometry the call would run on (ignored where the read takes the strips or the chain).  Key: one
// `value << key_bits | (2^key_bits - 1 - row)` per lane, where the largest possible value keeps it inside int16 (the bound of
// lane_key_ok, with this form's bits); Rows: a first-arg-max per row -- more than 16 rows per lane, or larger scores.  Chain:
// the banded block chain under band_placed = 1 (above), whatever the read length -- refused where the chain has no plan,
// never sent to the strips.  Wide: placed_wide = 1, unbanded -- the int32 sweep (placed_wide_kernels.hip.h) exactly where the rule
// would otherwise refuse for score_width = 32 or because the cells can leave int16 under score_width = 0 (16 means "int16 or
// refuse" and stays refused); whatever the read length, one pair per register.  Refused only where int32 cells could overflow.
inline PlacedChoice placed_choice(const RuleInputs &in, int alg, const PlacedFacts &f, int G, int K) {
    PlacedChoice c;
    (void)G;
    if (alg != kAlgSW)
        c.reason = "placed scores exist for Smith-Waterman only (the NW variant's score and its alignment's end cell are different cells)";
    else if (f.band_width > 0 && !f.band_placed)
        c.reason = "placed scores are not built for band_width > 0";
    else if (in.sse_policy)
        c.reason = "placed scores are not built for traceback_policy = 1 (SSE/AVX tie-breaks)";
    else if (f.band_width > 0) {
        // band_placed = 1: the chain or nothing -- the strips' band is the (160, 4) one, a different definition.  int32 cells
        // whatever score_width says, as for banded scores: neither score_width nor the int16 range rule is read here.
        if (!f.chain_usable)
            c.reason = "band_placed: the block chain has no usable plan for this read_length, ref_length, band_width and scoring (band_chain_plan); "
                       "placed scores under a band run nowhere else";
        else if (int32_refused(in))
            c.reason = "band_placed: shape x scoring can leave the int32 range of the DP cells";
        else if (!band_placed_key_ok(in))
            c.reason = "band_placed: min(read_length, ref_length) x match leaves the range of the chain's end-cell key (value << 4 in int32)";
        else {
            c.route = PlacedRoute::Chain;
            c.key_bits = kBandPlacedKeyBits;
        }
        return c;
    } else if (f.score_width == 32)
        c.reason = "placed scores are not built for score_width = 32 (int32 cells)";
    else if (!int16_range_ok(in, kAlgSW, true, false, 0))
        c.reason = "placed scores run on int16 cells: shape x scoring can leave their range";
    if (c.reason[0] && alg == kAlgSW && f.band_width <= 0 && !in.sse_policy && f.placed_wide && f.score_width != 16) {
        // one of the two int16 refusals just above, with the key on: int32 cells instead
        c.reason = "";
        if (int32_refused(in))
            c.reason = "placed_wide: shape x scoring can leave the int32 range of the DP cells";
        else
            c.route = PlacedRoute::Wide;
        return c;
    }
    if (c.reason[0]) return c;
    if (f.long_plan || (!f.forced && in.R > kPlacedStripRows)) {
        c.route = PlacedRoute::Strip;
        return c;
    }
    const int bits = placed_key_bits(K);
    const long long top = (long long)std::min(in.R, in.F) * std::max(in.sc.match, 0);
    if (K <= kPlacedKeyMaxK && ((top + 1) << bits) <= 32000) {
        c.route = PlacedRoute::Key;
        c.key_bits = bits;
    } else {
        c.route = PlacedRoute::Rows;
    }
    return c;
}

// describe()'s name of what the last placed call ran (ran_placed)
inline const char *ran_placed_name(PlacedRoute r) {
    static const char *const names[] = {"none", "key", "rows", "strip", "chain", "wide", "band"};
    return names[(int)r];
}

// ---- spanned scores (valign_hip_score_span_*): a placed score plus the begin cell, from a second sweep over the reversed
// prefixes that end in the end cell ----
// Reference columns the reverse sweep has to look back.  An alignment of score S >= 1 on a <= R read bases has d <= R diagonal
// columns and l columns that put a reference base against a gap in the read; with m = max(match, mismatch, 0) and c the
// cheapest price of one such gap base, S <= d m - l c, so l <= (R m - 1) / c and the alignment covers at most R + l columns.
// c = 0: no bound, F.  m = 0: no alignment scores at all, and min(R, F) columns hold every diagonal.
inline long long span_ref_length(const RuleInputs &in) {
    const Scoring &sc = in.sc;
    const long long R = in.R, F = in.F;
    const long long m = std::max({sc.match, sc.mismatch, 0});
    const long long c = sc.affine ? std::min(std::abs((long long)sc.open_read), std::abs((long long)sc.ext_read)) : std::abs((long long)sc.gap_read);
    if (c == 0) return F;
    const long long gap_cols = R * m >= 1 ? (R * m - 1) / c : 0;
    return std::min(F, R + gap_cols);
}

// A spanned call is two unbanded placed calls: refused exactly where placed_choice refuses one of those, with its texts -- and
// under a band whatever band_placed says: the chain's block windows are not symmetric under reversal, so the reverse sweep would
// run on another band than the forward one.  Otherwise the choice is the forward sweep's (the reverse sweep asks for its own
// shape, (R, span_ref_length)).  `G x K` as in placed_choice; without them only Refused or not, and the reason, mean anything.
inline PlacedChoice span_choice(const RuleInputs &in, int alg, const PlacedFacts &f, int G = 0, int K = 0) {
    PlacedFacts unbanded = f;
    unbanded.band_width = 0;
    PlacedChoice c = placed_choice(in, alg, unbanded, G, K);
    if (c.route != PlacedRoute::Refused && f.band_width > 0) {
        c = PlacedChoice{};
        c.reason = "spanned scores are not built for band_width > 0";
    }
    return c;
}

// ---- suboptimal scores (valign_hip_score_subopt_*): the placed record plus the best column maximum outside a window of
// `mask` reference columns around the end cell, from the placed register sweep alone ----
// A suboptimal call is an unbanded placed call on the register sweep: refused exactly where placed_choice refuses that, with
// its texts -- placed_wide does not open the int32 sweep here -- and, with texts of its own, for a negative mask, under a band
// whatever band_placed says, and where placed scores would leave the register sweep for the row strips (the column maxima
// ride the lane-to-lane hand-over of ONE sweep over all rows).  Otherwise Key or Rows, as placed_choice picks for `G x K`.
inline PlacedChoice subopt_choice(const RuleInputs &in, int alg, const PlacedFacts &f, int G, int K, int mask = 0) {
    PlacedFacts plain = f;
    plain.band_width = 0;
    plain.placed_wide = false;
    PlacedChoice c = placed_choice(in, alg, plain, G, K);
    if (c.route == PlacedRoute::Refused) return c;
    const char *reason = "";
    if (mask < 0)
        reason = "suboptimal scores need mask >= 0";
    else if (f.band_width > 0)
        reason = "suboptimal scores are not built for band_width > 0";
    else if (c.route != PlacedRoute::Key && c.route != PlacedRoute::Rows)
        reason = "suboptimal scores run on the register sweep only: reads of more than 1024 rows and shapes without a register geometry are refused";
    if (reason[0]) {
        c = PlacedChoice{};
        c.reason = reason;
    }
    return c;
}

// The sweep's suboptimal form adds a ring of `ring_bytes` to every wave's LDS, which the placed plan did not count: the waves
// of a block, `placed_waves` (the placed plan's) halved until the block's tables and rings fit `block_limit`; 0 where not even
// one wave's do, which is refused with kSuboptNoRing.
inline int subopt_block_waves(int wave_lds, int ring_bytes, int placed_waves, int block_limit) {
    for (int waves = placed_waves; waves >= 1; waves >>= 1)
        if ((long long)(wave_lds + ring_bytes) * waves <= block_limit) return waves;
    return 0;
}
constexpr const char *kSuboptNoRing = "suboptimal scores: one wave's reference tables leave no room for its column ring in the LDS (a shorter reference, or a geometry of more lanes per group, has it)";

// ---- extension scores (valign_hip_score_extend_*): the anchored score, its end cell and the read-end score, from one register
// sweep with gap-priced borders and no floor at zero (extend_kernels.hip.h) ----
// The cells are signed int16 and nothing clamps them from below, so the range is derived from the matrix itself:
//   * no cell is above min(R, F) * max(match, mismatch, 0): a path takes at most min(R, F) diagonal steps, nothing else adds;
//   * no cell of H is below the all-gaps path to the far corner -- R steps in the reference direction and F in the read
//     direction, each at its worst price (the path "down the border column, then along the row" reaches every cell and costs
//     at most that, since every gap score is <= 0);
//   * a candidate of a maximum (E, F, a diagonal) lies at most the largest single addend below an H.
// Both ends must stay within the +-32000 of int16_range_ok.
inline long long extend_cell_top(const RuleInputs &in) {
    return (long long)std::min(in.R, in.F) * std::max({in.sc.match, in.sc.mismatch, 0});
}
inline long long extend_cell_bottom(const RuleInputs &in) {
    const Scoring &sc = in.sc;
    const long long per_row = sc.affine ? std::min({sc.open_ref, sc.ext_ref, 0}) : std::min(sc.gap_ref, 0);
    const long long per_col = sc.affine ? std::min({sc.open_read, sc.ext_read, 0}) : std::min(sc.gap_read, 0);
    const long long addend = sc.affine ? std::min({sc.match, sc.mismatch, sc.open_read, sc.ext_read, sc.open_ref, sc.ext_ref, 0})
                                       : std::min({sc.match, sc.mismatch, sc.gap_read, sc.gap_ref, 0});
    return per_row * in.R + per_col * in.F + addend;
}
inline bool extend_int16_ok(const RuleInputs &in) { return extend_cell_top(in) <= 32000 && extend_cell_bottom(in) >= -32000; }

// extend_wide = 1: the same matrix on signed int32 cells (extend_wide_kernels.hip.h).  Nothing clamps them either, and the gap
// states of the two borders -- E of the border column, F of the border row -- are the finite sentinel kExtendWideLoses, which a
// step adds an extension score (<= 0) to like to any other cell: it drifts down, one extension per step.  With
// B = kExtendWideCellBound the call is legal where every cell and every candidate of a maximum lies in [-B, B]
// (extend_cell_top / extend_cell_bottom, above) and
//   * the sentinel plus any single addend -- the largest one a positive substitution score -- stays below -B, so below every real
//     cell and candidate: a value that derives from the sentinel loses every maximum a real value takes part in;
//   * the sentinel less (R + F) extensions at the worst price, and one more addend, stays inside int32: a sweep has fewer than
//     R + F steps, so no drift wraps round to a large value.
// Both hold for every scoring of int16 scores on shapes of R + F <= 32767 (2^28 > 2^15 and 2^29 + 2^15 x 2^15 + 2^15 < 2^31);
// they are tested all the same: the rule reads what it is given, not what the engine validates.
constexpr long long kExtendWideCellBound = 1ll << 28;
constexpr int kExtendWideLoses = -(1 << 29);
inline bool extend_int32_ok(const RuleInputs &in) {
    const Scoring &sc = in.sc;
    const long long top_addend = std::max({sc.match, sc.mismatch, 0});
    const long long worst_ext = sc.affine ? std::min({sc.ext_read, sc.ext_ref, 0}) : std::min({sc.gap_read, sc.gap_ref, 0});
    const long long low_addend = sc.affine ? std::min({sc.match, sc.mismatch, sc.open_read, sc.ext_read, sc.open_ref, sc.ext_ref, 0})
                                           : std::min({sc.match, sc.mismatch, sc.gap_read, sc.gap_ref, 0});
    if (extend_cell_top(in) > kExtendWideCellBound || extend_cell_bottom(in) < -kExtendWideCellBound) return false;
    if (kExtendWideLoses + top_addend >= -kExtendWideCellBound) return false;
    return kExtendWideLoses + worst_ext * ((long long)in.R + in.F) + low_addend >= -(1ll << 31);
}

// extend_band = 1 under a band: the int32 strip sweep over the block band on the anchor's diagonal (extend_band_plan.h has the
// band, include/valign_hip.h the definition).  Some cells are ABSENT, so the path "down the border column, then along the row" that
// extend_cell_bottom prices may not exist and the bottom of the cell range is derived again:
//   * every present cell holds the score of a monotone DIAG / UP / LEFT path from the origin through present cells (each present
//     cell has one: include/valign_hip.h);
//   * such a path has at most R steps down, at most F steps to the right and at most min(R, F) diagonal steps;
//   * a step down costs at worst min(open_ref, ext_ref, 0) (linear: min(gap_ref, 0)), a step right min(open_read, ext_read, 0)
//     (min(gap_read, 0)), a diagonal step min(match, mismatch, 0);
//   * so no cell of H lies below R * down + F * right + min(R, F) * diagonal, and a candidate of a maximum at most the largest
//     single addend below that.
// No cell is above extend_cell_top: a band only removes paths.  The sentinel kExtendWideLoses stands for every ABSENT neighbour as
// well as for the borders' gap states; a present cell always has a real candidate, so a sentinel-derived value is never stored
// in H and the sentinel conditions and the drift condition are those of extend_int32_ok, unchanged.
inline long long extend_band_cell_bottom(const RuleInputs &in) {
    const Scoring &sc = in.sc;
    const long long down = sc.affine ? std::min({sc.open_ref, sc.ext_ref, 0}) : std::min(sc.gap_ref, 0);
    const long long right = sc.affine ? std::min({sc.open_read, sc.ext_read, 0}) : std::min(sc.gap_read, 0);
    const long long diagonal = std::min({sc.match, sc.mismatch, 0});
    const long long addend = sc.affine ? std::min({sc.match, sc.mismatch, sc.open_read, sc.ext_read, sc.open_ref, sc.ext_ref, 0})
                                       : std::min({sc.match, sc.mismatch, sc.gap_read, sc.gap_ref, 0});
    return down * in.R + right * in.F + diagonal * std::min(in.R, in.F) + addend;
}
inline bool extend_band_int32_ok(const RuleInputs &in) {
    const Scoring &sc = in.sc;
    const long long top_addend = std::max({sc.match, sc.mismatch, 0});
    const long long worst_ext = sc.affine ? std::min({sc.ext_read, sc.ext_ref, 0}) : std::min({sc.gap_read, sc.gap_ref, 0});
    const long long low_addend = sc.affine ? std::min({sc.match, sc.mismatch, sc.open_read, sc.ext_read, sc.open_ref, sc.ext_ref, 0})
                                           : std::min({sc.match, sc.mismatch, sc.gap_read, sc.gap_ref, 0});
    if (extend_cell_top(in) > kExtendWideCellBound || extend_band_cell_bottom(in) < -kExtendWideCellBound) return false;
    if (kExtendWideLoses + top_addend >= -kExtendWideCellBound) return false;
    return kExtendWideLoses + worst_ext * ((long long)in.R + in.F) + low_addend >= -(1ll << 31);
}
constexpr const char *kExtendBandNoInt16 = "extend_band: banded extension scores run on int32 cells; score_width = 16 (int16 or refuse) is refused";
constexpr const char *kExtendBandRange = "extend_band: shape x scoring can leave the range the int32 cells keep below the sentinel of absent cells";

// An extension call runs on the register sweep's rows track or, under extend_wide = 1, on the int32 strip sweep: refused for the NW
// variant's mode bit, for traceback_policy = 1 and under a band whatever band_placed says -- whatever extend_wide says too.
// extend_wide = 0: refused as well for score_width = 32 whatever placed_wide says, where the cells could leave int16 (above), and
// for the shapes placed scores would send to the row strips; otherwise Rows.  extend_wide = 1: Wide exactly where one of those
// three refusals would stand (the int16 range one under score_width = 0 only: 16 means "int16 or refuse" and stays refused, as for
// placed scores) -- refused there, with a text of its own, only where extend_int32_ok fails; every other call decides as without
// the key.  extend_band = 1 qualifies "under a band": with band_width > 0 the call is Band -- the banded int32 strip sweep --
// whatever the read length, score_width 0 / 32 and extend_wide say, refused with texts of its own for score_width = 16 and where
// extend_band_int32_ok fails; the mode bit and traceback_policy = 1 keep their texts.  Without a band the key is not read.  `G x K`: the register geometry the call would run on -- every full geometry carries the four gap forms, so the choice
// does not depend on it today.
inline PlacedChoice extend_choice(const RuleInputs &in, int alg, const PlacedFacts &f, int G, int K) {
    PlacedChoice c;
    (void)G;
    (void)K;
    bool opens_wide = false;            // the refusal is one of the three extend_wide = 1 answers
    if (alg != kAlgSW)
        c.reason = "extension scores are defined for opt & 0xF == 0 only (the NW variant's free reference start is another matrix)";
    else if (in.sse_policy)
        c.reason = "extension scores are not built for traceback_policy = 1 (SSE/AVX tie-breaks)";
    else if (f.band_width > 0 && f.extend_band) {
        // extend_band = 1: the banded int32 strip sweep or nothing, whatever the read length and extend_wide say
        if (f.score_width == 16)
            c.reason = kExtendBandNoInt16;
        else if (!extend_band_int32_ok(in))
            c.reason = kExtendBandRange;
        else
            c.route = kPlacedRouteBand;
        return c;
    } else if (f.band_width > 0)
        c.reason = "extension scores are not built for band_width > 0";
    else if (f.score_width == 32) {
        c.reason = "extension scores are not built for score_width = 32 (int32 cells)";
        opens_wide = true;
    } else if (!extend_int16_ok(in)) {
        c.reason = "extension scores run on signed int16 cells: shape x scoring can leave their range";
        opens_wide = f.score_width == 0;
    } else if (f.long_plan || (!f.forced && in.R > kPlacedStripRows)) {
        c.reason = "extension scores run on the register sweep only: reads of more than 1024 rows and shapes without a register geometry are refused";
        opens_wide = true;
    } else
        c.route = PlacedRoute::Rows;
    if (opens_wide && f.extend_wide) {
        if (extend_int32_ok(in)) {
            c.reason = "";
            c.route = PlacedRoute::Wide;
        } else {
            c.reason = "extend_wide: shape x scoring can leave the range the int32 cells keep below their borders' sentinel";
        }
    }
    return c;
}

// ---- extension alignments (valign_hip_align_extend_*): the alignment from the anchor to the end cell the end-bonus rule picks, on
// the int16 register sweep with a back pointer per cell (extend_align_kernels.hip.h) ----
// An extension-alignment call is an extension call on the register sweep: refused exactly where extend_choice refuses with
// extend_wide = 0, with its texts; under extend_wide = 1, where extend_choice answers Wide (or refuses the int32 cells), refused
// with a text of its own -- the int32 / row-strip form has no back pointers.  Under a band with extend_band = 1: refused with
// kExtendAlignNoBand where the key off refuses for the band (the mode bit and traceback_policy = 1 come first, with their texts).
// Otherwise Rows, and the bytes of pointer stream a
// wave of the `G x K` geometry writes over `F` reference columns: ceil((F + G - 1) / 8) blocks of 8 steps, 64 lanes, K dwords per
// lane and block (linear gaps) or 2 K (affine: H codes and gap codes).  G = 0 (no register geometry): 0 bytes.
struct ExtendAlignChoice {
    PlacedRoute route = PlacedRoute::Refused;       // Rows or Refused
    const char *reason = "";                        // Refused: why
    int blocks8 = 0;                                // 8-step blocks per lane
    long long wave_ptr_bytes = 0;                   // pointer-scratch bytes of one wave
    int band_half = 0;                              // Band: w of the band (extend_band_plan.h), capped at the unbanded limit
};
// extend_band_align = 1 under a band with extend_band = 1 (include/valign_hip.h): the call is Band -- the banded int32 strip sweep
// with back pointers (extend_band_align_kernels.hip.h) -- wherever banded extension scores run, whatever the read length,
// score_width 0 / 32 and extend_wide say, and refused where they are refused, with their texts: the mode bit, traceback_policy = 1,
// score_width = 16 and the band's int32 range.  blocks8 and wave_ptr_bytes are then those of a pair-of-pairs -- the sweep's wave --
// over all strips, in the layout of extend_band_align_plan.h.  With the key off, without a band or without extend_band nothing
// below changes.
inline ExtendAlignChoice extend_band_align_choice(const RuleInputs &in, int alg, const PlacedFacts &f, int G, int K) {
    ExtendAlignChoice c;
    const PlacedChoice scores = extend_choice(in, alg, f, G, K);
    if (scores.route != kPlacedRouteBand) {
        c.reason = scores.reason;
        return c;
    }
    c.route = kPlacedRouteBand;
    c.band_half = extend_band_half(f.band_width, in.R, in.F);
    c.blocks8 = (int)extend_band_align_blocks_before(extend_band_align_strips(in.R), in.F, c.band_half);
    c.wave_ptr_bytes = extend_band_align_pp_dwords(in.R, in.F, c.band_half, in.sc.affine) * 4;
    return c;
}
constexpr const char *kExtendAlignNoWide = "extension alignments: not built for the int32 / row-strip route of extend_wide = 1 (the extension scores of this call run there)";
inline long long extend_align_wave_ptr_bytes(int G, int K, int F, bool affine) {
    if (G <= 0 || K <= 0) return 0;
    return (long long)((F + G - 1 + 7) / 8) * 64 * K * 4 * (affine ? 2 : 1);
}
constexpr const char *kExtendAlignNoBand = "extension alignments: not built under a band (extend_band = 1 runs the extension scores of this call on the banded int32 sweep, which keeps no back pointers)";
inline ExtendAlignChoice extend_align_choice(const RuleInputs &in, int alg, const PlacedFacts &f, int G, int K) {
    ExtendAlignChoice c;
    if (f.band_width > 0 && f.extend_band && f.extend_band_align) return extend_band_align_choice(in, alg, f, G, K);
    if (f.band_width > 0 && f.extend_band) {
        // the key off decides whether the band is what stands in the way: the mode bit and traceback_policy = 1 keep their texts
        PlacedFacts off = f;
        off.extend_band = false;
        off.extend_wide = false;
        const PlacedChoice plain = extend_choice(in, alg, off, G, K);
        c.reason = std::string(plain.reason) == "extension scores are not built for band_width > 0" ? kExtendAlignNoBand : plain.reason;
        return c;
    }
    const PlacedChoice scores = extend_choice(in, alg, f, G, K);
    if (f.extend_wide && scores.route != PlacedRoute::Rows) {
        PlacedFacts narrow = f;
        narrow.extend_wide = false;
        const PlacedChoice plain = extend_choice(in, alg, narrow, G, K);
        // the key changed the answer: the call's extension route is the wide one (or its int32 refusal)
        const bool wide = scores.route == PlacedRoute::Wide || std::string(scores.reason) != plain.reason;
        c.reason = wide ? kExtendAlignNoWide : plain.reason;
        return c;
    }
    if (scores.route != PlacedRoute::Rows) {
        c.reason = scores.reason;
        return c;
    }
    c.route = PlacedRoute::Rows;
    c.blocks8 = G > 0 ? (in.F + G - 1 + 7) / 8 : 0;
    c.wave_ptr_bytes = extend_align_wave_ptr_bytes(G, K, in.F, in.sc.affine);
    return c;
}

// ---- band_nw = 1: the NW variant under the block band (include/valign_hip.h) ----
// Consecutive blocks' windows connect -- every in-band cell has a present candidate -- once 2 * (band_width / 2) + 1 columns
// cover the most a window start advances per row, ceil(F / R).  Narrower bands are refused.
inline bool band_nw_connects(int R, int F, int band_width) {
    return R > 0 && 2ll * (band_width / 2) + 1 >= ((long long)F + R - 1) / R;
}
inline void band_nw_check(int R, int F, int band_width) {
    if (!band_nw_connects(R, F, band_width))
        throw std::runtime_error("band_nw: band_width " + std::to_string(band_width) + " is too narrow for read_length " + std::to_string(R) +
                                 ", ref_length " + std::to_string(F) + " (the windows of consecutive blocks do not connect: 2 * (band_width / 2) + 1 "
                                 "must be at least ceil(ref_length / read_length))");
}

// Banded NW-variant alignments on the packed int16 strips: an absent cell is the finite sentinel kBandNwAbsent16, forced at
// every cell outside its row's window, so it never drifts.  The sentinel is safe where
//   * sentinel + the largest addend (a profile value or a gap score) stays below every legitimate cell: a present cell is at
//     least the worst monotone in-band path to it from a border -- at most R + F + 2 steps, each the worst step score (affine:
//     E and F lie one more opening below an H);
//   * sentinel + the smallest addend does not wrap (the linear strips add without saturation);
//   * no legitimate cell exceeds 16000: the tracked row's first-arg-max test takes (running best - cell) in int16, and the
//     running best starts at the sentinel where the border column is absent.
inline bool band_nw_int16_ok(const RuleInputs &in) {
    const Scoring &sc = in.sc;
    const long long worst = sc.affine ? std::min({sc.open_read, sc.open_ref, sc.ext_read, sc.ext_ref, sc.mismatch, sc.match, 0})
                                      : std::min({sc.gap_read, sc.gap_ref, sc.mismatch, sc.match, 0});
    const long long top_add = std::max({sc.match, sc.mismatch, 0});
    const long long hi = (long long)std::min(in.R, in.F) * std::max(sc.match, 0) + 1;
    const long long lo = (long long)(in.R + in.F + 2) * worst + (sc.affine ? std::min({sc.open_read, sc.open_ref, 0}) : 0);
    return kBandNwAbsent16 + top_add < lo && kBandNwAbsent16 + worst >= -32768 && hi <= 16000;
}

// ---- the path of an alignment call ----
enum class AlignRoute { Fused, Register, Strip, StripBand, StripWide, StripWideBand, StripCkpt };

// What the route reads of the engine beyond the rule inputs (Engine::align_route)
struct RouteFacts {
    bool banded = false;            // band_alignments with a band_width
    bool wide_align = false;        // debug switch: int32 cells always
    bool read_strips = false;       // the alignment plan is the long-read one, or an unforced read of more than 1 024 rows
    bool fused_off = false;         // debug switch no_fused, or a forced geometry
    bool small_call = false;        // align_host's direct call: the one place the fused kernel is tried
    int fused_rows = 0;             // padded rows of the tallest fused geometry
    bool checkpoints = false;       // trace_checkpoints = 1: plain row strips keep checkpoint rows instead of every pointer
    bool band_nw = false;           // band_nw = 1: the band also applies to the NW variant
    int band_width = 0;             // ... whose calls are refused where the windows would not connect (band_nw_check)
};

// The cascade, once: refusals, then int32 cells, the band, row strips, the fused kernel for a small call, the register sweep.
// trace_checkpoints changes the memory of one path and nothing else: where the call would take the plain int16 row strips with
// the default tie-breaks it takes StripCkpt (same results); every other call runs as without the key.
// tagged_range_ok is asked about two different sweeps on purpose: Fused is decided before a fused geometry is picked, so it
// tests `fused_rows` (the tallest one: whichever geometry align_fused then takes is in range); the register path tests the
// rows of the plan it launches (fill_choice).
inline AlignRoute align_route(const RuleInputs &in, int alg, const RouteFacts &f) {
    if (f.banded && alg != kAlgSW && !f.band_nw) throw std::runtime_error("band_alignments applies to Smith-Waterman alignments only");
    if (f.banded && in.sse_policy)
        throw std::runtime_error("band_alignments needs traceback_policy = 0 (no banded SSE/AVX tie-breaks)");
    const bool nw_band = f.banded && alg == kAlgNW;
    if (nw_band) band_nw_check(in.R, in.F, f.band_width);
    // Alignments whose cells leave int16 (the reference's shorts would wrap): int32 cells on the row-strip path, one pair per
    // register (align_strip_wide_kernel) -- every mode
    // (the banded NW variant also where its int16 sentinel is not safe: band_nw_int16_ok)
    if (border_bad(in, alg) || !int16_range_ok(in, alg, false, false, 0) || f.wide_align || (nw_band && !band_nw_int16_ok(in))) {
        if (int32_refused(in))
            throw std::runtime_error("shape x scoring can leave the int32 range of the DP cells (read_length " + std::to_string(in.R) +
                                     ", ref_length " + std::to_string(in.F) + ")");
        return f.banded ? AlignRoute::StripWideBand : AlignRoute::StripWide;
    }
    // banded alignments: row strips that sweep the band windows (banded cells never exceed unbanded ones: the range
    // decision above stands)
    if (f.banded) return AlignRoute::StripBand;
    if (f.read_strips) return (f.checkpoints && !in.sse_policy) ? AlignRoute::StripCkpt : AlignRoute::Strip;
    if (in.sse_policy && in.sc.affine)
        throw std::runtime_error("traceback_policy = 1 (SSE/AVX tie-breaks) exists for the linear gap model only");
    // fill + traceback in one launch: linear gaps, default tie-breaks, plain tagged cells
    if (f.small_call && !f.fused_off && !in.sc.affine && !in.sse_policy && !in.no_tag && tagged_range_ok(in, alg, f.fused_rows)) return AlignRoute::Fused;
    return AlignRoute::Register;
}

// align_host sizes its chunks for strips where the read or the band asks for them; int32 cells alone (a short read whose
// cells leave int16) keep the register path's chunks
inline bool strip_chunks(AlignRoute r, const RouteFacts &f) {
    return r == AlignRoute::Strip || r == AlignRoute::StripCkpt || r == AlignRoute::StripBand || r == AlignRoute::StripWideBand || (r == AlignRoute::StripWide && f.read_strips);
}

// describe()'s name of what an alignment call launched (ran_align_fill); fill_kernel: the register path's FillKernel
inline const char *ran_fill_name(AlignRoute r, int fill_kernel = -1) {
    static const char *const names[kFillKernels] = {"linear", "linear_sym", "affine", "sse", "tag", "tag_key", "affine_sym",
                                                    "affine_tag", "affine_tag_sym", "sse_tag", "sse_tag_key", "tag_prof_key"};
    static const char *const routes[] = {"fused_tag", nullptr, "strip", "strip_band", "strip_wide", "strip_wide_band", "strip_ckpt"};     // by AlignRoute
    if (r != AlignRoute::Register) return routes[(int)r];
    return fill_kernel >= 0 && fill_kernel < kFillKernels ? names[fill_kernel] : "none";
}

// ---- spanned CIGARs (valign_hip_align_span_*): the alignment of the span, filled and walked on the span's window ----
// A spanned CIGAR call is a spanned call whose reverse sweep is an ALIGNMENT of the child shape (R, span_ref_length): refused
// exactly where span_choice refuses, with its texts, and where align_route refuses the child's call, that text prefixed with
// "spanned CIGARs: ".  Asked before anything is staged or launched.  `child` / `child_facts`: the rule inputs and route facts of
// the child engine (Engine::span_cigar_prepare); `G x K` as in span_choice.
struct SpanCigarChoice {
    PlacedChoice forward;                       // the forward sweep's choice (route Refused: see reason)
    AlignRoute child = AlignRoute::Register;    // the route of the child's alignment call, where nothing is refused
    std::string reason;                         // why the call is refused; empty where it is not
    bool refused() const { return !reason.empty(); }
};
constexpr const char *kSpanCigarPrefix = "spanned CIGARs: ";
inline SpanCigarChoice span_cigar_choice(const RuleInputs &in, int alg, const PlacedFacts &f, const RuleInputs &child, const RouteFacts &child_facts,
                                         int G = 0, int K = 0) {
    SpanCigarChoice c;
    c.forward = span_choice(in, alg, f, G, K);
    if (c.forward.route == PlacedRoute::Refused) {
        c.reason = c.forward.reason;
        return c;
    }
    try {
        c.child = align_route(child, alg, child_facts);
    } catch (const std::runtime_error &e) {
        c.forward = PlacedChoice{};
        c.reason = std::string(kSpanCigarPrefix) + e.what();
    }
    return c;
}

}  // namespace valign
