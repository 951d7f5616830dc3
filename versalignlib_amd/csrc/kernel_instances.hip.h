// kernel_instances.hip.h -- which (G, K) geometries exist, which kernels each one carries, and in which translation
// unit they are compiled.  The plugin is one shared object, but several hundred kernel instances in one hipcc run take
// minutes: the engine units only declare them (extern template), kernel_part.hip is compiled once per part
// (-DVALIGN_PART=n, in parallel, versalignlib_amd/build.py) and defines them.
//
// Round 4 pruned the table to what the engine can select (21 geometries x 35 kernels = 735 instances before):
//   * 17 geometries: 8x16, 8x20, 16x16 and 32x16 never win the cost model (Engine::choose_plan) -- a geometry of the
//     same row capacity with ~10 rows per lane is cheaper at every shape, for throughput and for latency;
//   * every geometry carries the 14 score kernels and the 5 alignment-fill kernels the engine picks for ordinary
//     scorings with the default tie-breaks (tagged cells; symmetric affine scores: VALIGN_FAST_KERNELS);
//   * everything else -- the equality-test fill kernels (the fallback for scorings whose tagged cells would leave int16,
//     and for the debug switch no_tag), the per-row arg-max forms, the SSE2 / AVX2 tie-break kernels and affine
//     alignments with different scores per direction -- exists for SIX geometries only, one per row capacity (64, 160,
//     320, 512, 1024, 2048); a call that needs one of them on another geometry is re-planned onto the next full one
//     (Engine::align_plan_for): same results, a sweep a few per cent longer.
// Placed scores (placed_kernels.hip.h) add 68 instances, listed by placed_kernel<G, K, FULL> there: the symmetric gap forms with
// the lane key on the 15 geometries of up to 16 rows per lane, the asymmetric ones on the five full geometries among them, and
// the four per-row forms on the six full geometries and 64 x 24.  VALIGN_PLACED_KERNELS instantiates a geometry's table.
// Two instances are compiled but unselectable: SW tag_prof_key on 64 x 24 and 64 x 32 (prof_key_ok, cell_rules.h, needs K <= 16).
// ONE SIDE GEOMETRY stands outside the table: 8 x 19, 152 rows, with ONE kernel -- score_kernel<8, 19, kAlgSW, kGapAffineSym>, the
// tilted sweep's row-table forms (cell_constants.h: tilt_tables_only).  It is not an 18th geometry: no fill, placed, suboptimal or
// extension kernel exists for it, nothing is re-planned onto it, and the counts above (17 geometries, 68 / 44 / 24) stand.  The
// engine takes it for int16 symmetric affine Smith-Waterman scores of reads of 129 .. 152 bases where cell_rules.h:
// sym_affine_side_tile_refusal has nothing to refuse.  VALIGN_SIDE_KERNELS names it; it is compiled in part VALIGN_SIDE_PART, the
// lightest one (part 1 finishes first and is the smallest object).
#pragma once

#include "dp_kernels.hip.h"
#include "trace_kernels.hip.h"
#include "placed_kernels.hip.h"
#include "extend_kernels.hip.h"
#include "extend_align_kernels.hip.h"

// X(G, K): geometries with every kernel;  Y(G, K): geometries with the fast set only.  Parts are balanced by rows per
// lane (compile time grows with K).
#define VALIGN_PART0(X, Y) X(64, 32) Y(8, 4)
#define VALIGN_PART1(X, Y) Y(64, 24) Y(8, 6) Y(16, 4)
#define VALIGN_PART2(X, Y) X(64, 16) Y(8, 10)
#define VALIGN_PART3(X, Y) X(16, 10) Y(8, 12) Y(16, 8)
#define VALIGN_PART4(X, Y) X(32, 10) Y(16, 12) Y(64, 12)
#define VALIGN_PART5(X, Y) X(64, 8) X(8, 8) Y(32, 8) Y(32, 12)
#define VALIGN_KERNEL_PARTS 6
#define VALIGN_SIDE_PART 1
#define VALIGN_SIDE_KERNELS(PREFIX) PREFIX __global__ void score_kernel<kSideTileG, kSideTileK, kAlgSW, kGapAffineSym>(const ScoreArgs);

#define VALIGN_ALL_PARTS(X, Y) VALIGN_PART0(X, Y) VALIGN_PART1(X, Y) VALIGN_PART2(X, Y) VALIGN_PART3(X, Y) VALIGN_PART4(X, Y) VALIGN_PART5(X, Y)

// The kernels every geometry has; PREFIX is `extern template` (declaration) or `template` (definition).
#define VALIGN_FAST_KERNELS(PREFIX, G, K)                                                            \
    PREFIX __global__ void score_kernel<G, K, kAlgSW, kGapLinear>(const ScoreArgs);                  \
    PREFIX __global__ void score_kernel<G, K, kAlgSW, kGapSym>(const ScoreArgs);                     \
    PREFIX __global__ void score_kernel<G, K, kAlgSW, kGapAffine>(const ScoreArgs);                  \
    PREFIX __global__ void score_kernel<G, K, kAlgSW, kGapAffineSym>(const ScoreArgs);               \
    PREFIX __global__ void score_kernel<G, K, kAlgSW, kGapAffineSymF16>(const ScoreArgs);            \
    PREFIX __global__ void score_kernel<G, K, kAlgSW, kGapAffineF16>(const ScoreArgs);               \
    PREFIX __global__ void score_kernel<G, K, kAlgNW, kGapLinear>(const ScoreArgs);                  \
    PREFIX __global__ void score_kernel<G, K, kAlgNW, kGapSym>(const ScoreArgs);                     \
    PREFIX __global__ void score_kernel<G, K, kAlgNW, kGapAffine>(const ScoreArgs);                  \
    PREFIX __global__ void score_kernel<G, K, kAlgNW, kGapAffineSym>(const ScoreArgs);               \
    PREFIX __global__ void score_kernel<G, K, kAlgNW, kGapAffineSymF16>(const ScoreArgs);            \
    PREFIX __global__ void score_kernel<G, K, kAlgNW, kGapAffineF16>(const ScoreArgs);               \
    PREFIX __global__ void score_kernel<G, K, kAlgNW, kGapSymF16>(const ScoreArgs);                  \
    PREFIX __global__ void score_kernel<G, K, kAlgSW, kGapSymF16>(const ScoreArgs);                  \
    PREFIX __global__ void align_fill_affine_tag_kernel<G, K, kAlgSW, true>(const FillArgs);         \
    PREFIX __global__ void align_fill_affine_tag_kernel<G, K, kAlgNW, true>(const FillArgs);         \
    PREFIX __global__ void align_fill_tag_kernel<G, K, kAlgSW, true, false>(const FillArgs);         \
    PREFIX __global__ void align_fill_tag_kernel<G, K, kAlgSW, true, false, false, true>(const FillArgs); \
    PREFIX __global__ void align_fill_tag_kernel<G, K, kAlgNW, false, false>(const FillArgs);

// ... and what only the full geometries add: equality-test pointer kernels and the per-row arg-max forms of the tagged ones
#define VALIGN_FALLBACK_KERNELS(PREFIX, G, K)                                                        \
    PREFIX __global__ void align_fill_kernel<G, K, kAlgSW, false>(const FillArgs);                   \
    PREFIX __global__ void align_fill_kernel<G, K, kAlgSW, true>(const FillArgs);                    \
    PREFIX __global__ void align_fill_kernel<G, K, kAlgNW, false>(const FillArgs);                   \
    PREFIX __global__ void align_fill_kernel<G, K, kAlgNW, true>(const FillArgs);                    \
    PREFIX __global__ void align_fill_affine_kernel<G, K, kAlgSW, false>(const FillArgs);            \
    PREFIX __global__ void align_fill_affine_kernel<G, K, kAlgNW, false>(const FillArgs);            \
    PREFIX __global__ void align_fill_affine_kernel<G, K, kAlgSW, true>(const FillArgs);             \
    PREFIX __global__ void align_fill_affine_kernel<G, K, kAlgNW, true>(const FillArgs);             \
    PREFIX __global__ void align_fill_sse_kernel<G, K, kAlgSW>(const FillArgs);                      \
    PREFIX __global__ void align_fill_sse_kernel<G, K, kAlgNW>(const FillArgs);                      \
    PREFIX __global__ void align_fill_tag_kernel<G, K, kAlgSW, false, false>(const FillArgs);        \
    PREFIX __global__ void align_fill_tag_kernel<G, K, kAlgSW, false, true>(const FillArgs);         \
    PREFIX __global__ void align_fill_tag_kernel<G, K, kAlgSW, true, true>(const FillArgs);          \
    PREFIX __global__ void align_fill_tag_kernel<G, K, kAlgNW, false, true>(const FillArgs);         \
    PREFIX __global__ void align_fill_affine_tag_kernel<G, K, kAlgSW, false>(const FillArgs);        \
    PREFIX __global__ void align_fill_affine_tag_kernel<G, K, kAlgNW, false>(const FillArgs);

// The placed-score kernels of a geometry: defined where its table is (FULL: the geometry is a full one)
#define VALIGN_PLACED_KERNELS(PREFIX, G, K, FULL) PREFIX const void *placed_kernel<G, K, FULL>(int, int);

// The suboptimal-score kernels (placed_kernels.hip.h: subopt_kernel<G, K, FULL>, the SUB form of score_placed_kernel): 44 instances,
// all on the six full geometries
#define VALIGN_SUBOPT_KERNELS(PREFIX, G, K, FULL) PREFIX const void *subopt_kernel<G, K, FULL>(int, int);

// The extension-score kernels (extend_kernels.hip.h: extend_kernel<G, K, FULL>, score_extend_kernel): the four gap forms on the six
// full geometries, 24 instances
#define VALIGN_EXTEND_KERNELS(PREFIX, G, K, FULL) PREFIX const void *extend_kernel<G, K, FULL>(int);
// ... and their ZDROP forms (extend_zdrop_kernel<G, K, FULL>: keys extend_zdrop > 0 and extend_zdrop_rows = 1), 24 more
#define VALIGN_EXTEND_ZDROP_KERNELS(PREFIX, G, K, FULL) PREFIX const void *extend_zdrop_kernel<G, K, FULL>(int); PREFIX const void *extend_align_zdrop_kernel<G, K, FULL>(int);

// The extension-alignment fills (extend_align_kernels.hip.h: extend_align_kernel<G, K, FULL>, align_extend_fill_kernel): linear and
// affine gaps on the six full geometries, 12 instances (and 12 ZDROP forms: extend_align_zdrop_kernel<G, K, FULL>, above)
#define VALIGN_EXTEND_ALIGN_KERNELS(PREFIX, G, K, FULL) PREFIX const void *extend_align_kernel<G, K, FULL>(int);
