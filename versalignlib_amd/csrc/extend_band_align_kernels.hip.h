// extend_band_align_kernels.hip.h -- banded extension alignments (key extend_band_align; include/valign_hip.h has the definition,
// tests/extend_band_align_ref.py restates it): the alignment of an extension inside the block band on the anchor's diagonal, from
// the anchor to the end cell the end-bonus rule picks, on int32 cells and 512-row strips -- whatever the read length.
//
// Three kernels, one launch per strip of the first, then one each:
//   align_extend_band_fill_kernel   the BANDED score_extend_wide_kernel sweep (extend_wide_kernels.hip.h) instantiated with its
//                                   PTRS parameter -- the per-lane window, the sentinel for absent neighbours, the stale boundary-row
//                                   columns, the border row from column w, the early returns and the partial records across strips
//                                   are that sweep's, instruction for instruction -- which also derives every cell's back pointer
//                                   by the equality tests of align_extend_fill_kernel (extend_align_kernels.hip.h) on int32 cells
//                                   and streams the codes to HBM in the layout of extend_band_align_plan.h.
//                                   StripArgs of this sweep: ptr = the partial records, first_bad = the trimmed lengths, ends =
//                                   the chunk's pointer regions (dwords).
//   extend_band_ends_kernel         after the last strip: the merged partial records -> the extension record (the closed-form
//                                   unreached case of extend_wide_records_kernel), written to d_extend where asked, and the
//                                   EndCell the walk starts from, by the end-bonus rule in 64 bits.
//   extend_band_walk_kernel         one lane per pair: extend_walk_kernel's loop (extend_walk_pair) with the plan's addressing.
//                                   cigar_encode_kernel reads its rows unchanged.
//
// Codes: those of the register form.  Linear: 0 DIAG, 1 UP, 2 LEFT.  Affine: the H word 0 DIAG / 1 vertical / 2 horizontal state,
// the gap word bit 0 "the vertical state was extended", bit 1 "the horizontal state was extended"; an open wins a tie.
// Places that go wrong silently:
//   ABSENT CANDIDATES  an absent neighbour is the sentinel kExtendWideLoses (or a value drifted down from it); a present cell
//     always has a present candidate and extend_band_int32_ok keeps every cell above the sentinel's range, so a cell never EQUALS
//     a sentinel-derived candidate and the walk never leaves the band.  Gap bits of a state whose value is sentinel-derived are
//     garbage, and never read: the walk enters a state only where the cell equals it.
//   HALVES  the two pairs of a wave share a dword: the per-step shift clears the two bits that would cross from pair A's half
//     into pair B's, and so does the move of a short last block.
//   SHORT LAST BLOCK  a strip's steps need not be a multiple of 8: the last block's codes are moved up so that step t lies at
//     2 * (7 - (t & 7)) as in every other block.
//   REGIONS  are sized for the engine's F; a wave whose larger Fp is smaller writes the first blocks only, a strip below both Rp
//     or with an empty window writes none -- no walk reads there: a path never moves right or down.  Under extend_zdrop a strip
//     that a wave skips (both pairs dropped above it) writes no block either: the walk starts above T, from the best cell among the
//     rows before it -- a dropped pair's read end is unreached and never chosen -- and only moves up and left, so it never reads one.
//   DON'T-CARE BITS  steps outside a lane's window leave the codes of no cell; they are stored and never read.
#pragma once

#include "extend_align_kernels.hip.h"
#include "extend_wide_kernels.hip.h"

namespace valign {

// The fill: the sweep's kernel with BANDED and PTRS (two instances: linear and affine gaps at K = 8)
template <int K, bool AFFINE>
constexpr auto align_extend_band_fill_kernel = &score_extend_wide_kernel<K, AFFINE, true, true>;
// ... and under extend_zdrop (extend_zdrop.h): the same with ZDROP
template <int K, bool AFFINE>
constexpr auto align_extend_band_fill_zdrop_kernel = &score_extend_wide_kernel<K, AFFINE, true, true, true>;

#ifdef VALIGN_TU_EXTEND_ALIGN      // not templates: defined once, in engine_extend_align.hip
// One lane per pair.  partial / lens: what the strips and extend_wide_lengths_kernel left (extend_wide_kernels.hip.h).
// drop_rows (null: the key extend_zdrop is off): the read end of a pair that dropped is unreached, and so never chosen.
__global__ void __launch_bounds__(256)
extend_band_ends_kernel(const int *partial, const int *lens, ExtendRec *extend, EndCell *ends, long long n, int band_half, int end_bonus, const int *drop_rows) {
    const long long pair = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pair >= n) return;
    const int *rec = partial + kExtendWideRecDwords * pair;
    const int Rp = lens[2 * pair];
    const bool empty = Rp == 0;
    // the strip that holds row Rp - 1 may have returned before it wrote the pair: the unreached read end in closed form
    const bool unreached = extend_band_unreached(Rp, lens[2 * pair + 1], band_half) || (drop_rows && extend_zdrop_unreached(drop_rows[pair], Rp));
    ExtendRec r;
    r.score = empty ? 0 : rec[0];
    r.read_end = empty ? 0 : rec[1];
    r.ref_end = empty ? 0 : rec[2];
    r.gscore = empty ? 0 : (unreached ? VALIGN_HIP_EXTEND_UNREACHED : rec[3]);
    r.gref_end = empty || unreached ? 0 : rec[4];
    if (extend) extend[pair] = r;
    // the end-bonus rule in 64 bits.  An unreached read end is never chosen: INT32_MIN + INT32_MAX = -1 < 0 <= score
    EndCell start{-1, -1, 0, 0};                                    // the empty alignment
    int value = 0;
    if (!empty && end_bonus >= 0 && (long long)r.gscore + end_bonus >= (long long)r.score) {
        start.read_pos = (short)(Rp - 1);                           // (coordinates fit a short: R + F <= 32767)
        start.ref_pos = (short)(r.gref_end - 1);
        value = r.gscore;
    } else if (!empty && r.score > 0) {
        start.read_pos = (short)(r.read_end - 1);
        start.ref_pos = (short)(r.ref_end - 1);
        value = r.score;
    }
    start.score = (short)(value & 0xFFFF);                          // (low and high half of the int32 value, as align_strip_wide_kernel leaves it)
    start.pad = (short)(value >> 16);
    ends[pair] = start;
}

// The plan's addressing for extend_walk_pair: the strip's base and t_begin are kept while the walk stays in a strip (it leaves
// each strip once, upwards).
struct ExtendBandWalkLayout {
    int F, w;
    bool affine;
    int strip = -1, t_begin = 0;
    long long base = 0;
    static constexpr int kGapWord = kExtendBandBlockRows;
    __device__ long long word(int i, int j, int &t) {
        const int s = i / kExtendBandStripRows, in_strip = i - s * kExtendBandStripRows;
        if (s != strip) {
            strip = s;
            base = extend_band_align_strip_base(s, F, w, affine);
            t_begin = extend_band_strip(s, F, w).t_begin;
        }
        const int l = in_strip / kExtendBandBlockRows, q = in_strip - l * kExtendBandBlockRows;
        t = j + l;
        return base + extend_band_align_word((t - t_begin) / kExtendBandAlignBlockSteps, l, q, affine);
    }
};

// ExtendWalkArgs of this walk: ptr = the chunk's pointer regions, blocks8 = the 8-step blocks of a pair-of-pairs' region (all
// strips), band_half = w; G and K are not read.
__global__ void __launch_bounds__(256)
extend_band_walk_kernel(const ExtendWalkArgs a) {
    const long long pair = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= a.n) return;
    const long long pp_dwords = (long long)a.blocks8 * 64 * extend_band_align_lane_dwords(a.affine != 0);
    ExtendBandWalkLayout layout{a.F, a.band_half, a.affine != 0};
    extend_walk_pair(a, pair, a.ptr + (pair >> 1) * pp_dwords, pp_dwords, layout);
}
#endif

}  // namespace valign
