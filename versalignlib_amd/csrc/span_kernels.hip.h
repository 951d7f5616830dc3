// span_kernels.hip.h -- the two kernels of the spanned scores (include/valign_hip.h: valign_hip_span; engine_span.hip) around
// the two placed-score sweeps: the reversal of the prefixes that end in the end cell, and the records.
//
// A spanned score is the placed record plus the cell where the best local alignment BEGINS.  The end cell is the only cell of
// the prefix rectangle read[0, read_end) x ref[0, ref_end) that holds the score, so the same Smith-Waterman sweep over the two
// REVERSED prefixes has the score as its maximum exactly in the cells where an optimal alignment can begin; its first such cell
// in row-major order -- an ordinary placed record of the reversed pair -- is the begin cell.  The reversed reference is clipped
// to span_ref_length (cell_rules.h) columns: no alignment of a positive score reaches further back.
//
// Both kernels are bandwidth-bound and hold no DP.  Byte loads and byte stores, consecutive lanes on consecutive bytes (the
// aligned-dword forms of the ragged copy kernels were slower than their byte forms; nothing cleverer has been measured here).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "placed_kernels.hip.h"

namespace valign {

struct SpanRec {              // = valign_hip_span (include/valign_hip.h), 20 bytes
    int score, read_begin, read_end, ref_begin, ref_end;
};

struct SpanReverseArgs {
    const uint8_t *reads;     // n * R bytes, pair-major
    const uint8_t *refs;      // n * F bytes, pair-major
    const PlacedRec *fwd;     // n forward records
    uint8_t *rev_reads;       // n * R bytes: the reversed read prefix, then NUL
    uint8_t *rev_refs;        // n * Fr bytes: the first Fr bytes of the reversed reference prefix, then NUL
    long long n;
    int R, F, Fr;
    int pairs_per_block;      // consecutive pairs of one block: pairs_per_block * max(R, Fr) stays inside int
};

__device__ __forceinline__ int span_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

#ifdef VALIGN_TU_SPAN      // not templates: defined once, in engine_span.hip
// rev_reads[p][k] = reads[p][read_end - 1 - k] for k < read_end, rev_refs[p][k] = refs[p][ref_end - 1 - k] for
// k < min(ref_end, Fr), NUL elsewhere.  A block takes pairs_per_block consecutive pairs, whose destination bytes are one
// contiguous range of each buffer: thread t writes bytes t, t + 256, ... of it.  read_end / ref_end are clamped to [0, R] /
// [0, F] before they index anything: a wrong record gives a wrong answer, never an address outside the pair's sequences.
__global__ void __launch_bounds__(256)
span_reverse_kernel(const SpanReverseArgs a) {
    const long long pair0 = (long long)blockIdx.x * a.pairs_per_block;
    if (pair0 >= a.n) return;
    const int cnt = (int)(a.n - pair0 < a.pairs_per_block ? a.n - pair0 : a.pairs_per_block);
    const PlacedRec *fwd = a.fwd + pair0;
    if (a.R > 0) {
        const uint8_t *src = a.reads + (size_t)pair0 * a.R;
        uint8_t *dst = a.rev_reads + (size_t)pair0 * a.R;
        const unsigned total = (unsigned)cnt * (unsigned)a.R;
        for (unsigned at = threadIdx.x; at < total; at += 256) {
            const unsigned p = at / (unsigned)a.R;
            const int k = (int)(at - p * (unsigned)a.R);
            const int end = span_clamp(fwd[p].read_end, a.R);
            dst[at] = k < end ? src[(size_t)p * a.R + (end - 1 - k)] : (uint8_t)0;
        }
    }
    if (a.Fr > 0) {
        const uint8_t *src = a.refs + (size_t)pair0 * a.F;
        uint8_t *dst = a.rev_refs + (size_t)pair0 * a.Fr;
        const unsigned total = (unsigned)cnt * (unsigned)a.Fr;
        for (unsigned at = threadIdx.x; at < total; at += 256) {
            const unsigned p = at / (unsigned)a.Fr;
            const int k = (int)(at - p * (unsigned)a.Fr);
            const int end = span_clamp(fwd[p].ref_end, a.F);          // (Fr <= F: k < end keeps end - 1 - k inside [0, F))
            dst[at] = k < end ? src[(size_t)p * a.F + (end - 1 - k)] : (uint8_t)0;
        }
    }
}

// Forward and reverse record -> the 20-byte record: begin = end - reverse end; score and ends are the forward sweep's; five
// zeros where the forward score is 0.
__global__ void __launch_bounds__(256)
span_records_kernel(const PlacedRec *fwd, const PlacedRec *rev, SpanRec *spans, long long n) {
    const long long pair = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pair >= n) return;
    const PlacedRec f = fwd[pair], r = rev[pair];
    SpanRec s{0, 0, 0, 0, 0};
    if (f.score > 0) {
        s.score = f.score;
        s.read_begin = f.read_end - r.read_end;
        s.read_end = f.read_end;
        s.ref_begin = f.ref_end - r.ref_end;
        s.ref_end = f.ref_end;
    }
    spans[pair] = s;
}
#endif

}  // namespace valign
