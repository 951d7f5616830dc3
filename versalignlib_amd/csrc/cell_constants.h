// cell_constants.h -- what the kernels' template arguments and the host's choice of them (cell_rules.h) both name: the scoring
// of an engine, the algorithms, the gap forms of the score kernels and the fill kernels of a geometry.  No HIP here.
#pragma once

namespace valign {

struct Scoring {
    int match = 2, mismatch = -1, gap_read = -3, gap_ref = -3;
    bool affine = false;
    int open_read = -3, ext_read = -3, open_ref = -3, ext_ref = -3;
};

constexpr int kAlgSW = 0;
constexpr int kAlgNW = 1;

// GAPS of score_kernel selects the recurrence (dp_kernels.hip.h describes each form)
constexpr int kGapLinear = 0, kGapSym = 1, kGapAffine = 2, kGapAffineSym = 3;       // int16 cells
constexpr int kGapAffineSymF16 = 4, kGapAffineF16 = 5, kGapSymF16 = 6;              // the same recurrences on half floats
// The tilted biased form of kGapAffineSym (Smith-Waterman) unrolls its steady loop K steps deep: built for K <= 12 (at 16, 24
// or 32 rows per lane one trip is tens of KB of code); the rule sym_affine_tilt_ok (cell_rules.h) reads the same constant
constexpr int kTiltMaxK = 12;
// ... and for ONE tile beyond that, 8 lanes x 19 rows: 152 rows, the tile that fits reads of 129 .. 152 bases into a wave64 with
// 1.3 % padding (16 x 10: 160 rows).  It is a side geometry (engine.hip.h: kSideGeometry) with one kernel,
// score_kernel<8, 19, kAlgSW, kGapAffineSym>, and that kernel carries the tilted sweep's row-table forms only: an odd K has no
// K / 2 dwords of profile per lane, so nothing of the LDS profile is built for it.  The trait admits it by name; kTiltMaxK stays
// (raising it would put the tilted sweep into 64 x 16).
constexpr int kSideTileG = 8, kSideTileK = 19;
constexpr bool tilt_tables_only(int G, int K) { return G == kSideTileG && K == kSideTileK; }
constexpr bool tilt_frame_built(int G, int K) { return K <= kTiltMaxK || tilt_tables_only(G, K); }
// LDS of one wave of that tile over R x F (dp_kernels.hip.h lays it out: wave_setup_tables, row_table_lds16): the 16 raw references,
// then 8 selector streams of 16 bits per column with F + 2 x 12 pad columns each, the raw reads staged where the streams are built
// afterwards.  The group stride is 8 (mod 64) dwords.  Defined here so that the rule that budgets it (cell_rules.h) and the
// kernel's host side read one arithmetic.
constexpr int kSideTilePad = kSideTileG + 4, kSideTilePairs = 2 * (64 / kSideTileG);
constexpr int side_tile_refs_area(int F) { return ((kSideTilePairs * F + 32 + 15) / 16) * 16; }
constexpr int side_tile_stream_stride(int F) {              // bytes of one group's stream
    const int dw = (F + 2 * kSideTilePad + 1) / 2;
    return 4 * (dw + ((kSideTileG - dw) % 64 + 64) % 64);
}
constexpr int side_tile_wave_lds(int R, int F) {
    const int streams = (64 / kSideTileG) * side_tile_stream_stride(F), raw_reads = ((kSideTilePairs * R + 32 + 15) / 16) * 16;
    return side_tile_refs_area(F) + (streams > raw_reads ? streams : raw_reads);
}

// band_nw: what an ABSENT cell holds on the packed int16 strips (= kNegInf, the "minus infinity" of the affine NW borders;
// band_nw_int16_ok, cell_rules.h, says where it is safe) and on int32 cells (chain, strips: -2^29)
constexpr int kBandNwAbsent16 = -16384;
constexpr int kBandNwAbsent32 = -(1 << 29);

// alignment fill kernels of a geometry, by what the engine selects (fill_choice, cell_rules.h)
enum FillKernel {
    kFillLinear = 0,        // equality-test pointers, two gap scores            (full geometries only)
    kFillLinearSym,         // ... one shared gap score                           (full)
    kFillAffine,            // affine, equality tests                             (full)
    kFillSse,               // SSE2 / AVX2 tie-breaks, equality tests             (full)
    kFillTag,               // pointer tagged into the cell; SW: per-row arg-max  (NW: every geometry; SW: full)
    kFillTagKey,            // ... SW with one end-cell key per lane              (every geometry)
    kFillAffineSym,         // affine with symmetric scores, equality tests       (full)
    kFillAffineTag,         // affine, tagged cells, different scores per direction (full)
    kFillAffineTagSym,      // ... symmetric scores                               (every geometry)
    kFillSseTag,            // SSE tie-breaks, tagged; SW: per-row arg-max        (full)
    kFillSseTagKey,         // ... SW with the lane key                           (full)
    kFillTagProfKey,        // SW, the end-cell key rides in the query profile    (every geometry)
    kFillKernels
};

}  // namespace valign
