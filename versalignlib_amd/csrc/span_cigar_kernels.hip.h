// span_cigar_kernels.hip.h -- the backward encoder of the spanned CIGARs (include/valign_hip.h: valign_hip_align_span_*;
// engine_span_cigar.hip).
//
// A spanned CIGAR is the alignment of the two REVERSED prefixes that end in the pair's end cell, filled and walked by a child
// engine of shape (R, span_ref_length).  The child's walk leaves right-justified gapped rows in the reversed frame: column
// `end - 1` of those rows is the alignment's FIRST column in forward reading order.  This encoder is cigar_encode_kernel
// (cigar_kernels.hip.h) read the other way: per step lane l takes column end - 1 - (s * W + l), so consecutive lanes hold
// consecutive columns of the FORWARD alignment and the runs come out in forward reading order directly -- no reverse-order op
// buffer, no second pass.  Column rule, run lengths, the lane-group scheme (16 or 64 lanes per pair, a ballot of run
// boundaries, a carried open run) and the count-pass / emit-pass forms are cigar_encode_kernel's.  The affine open / extend
// choice keys on the previous op in reading order, as there: a run's first column pays the open price in either direction.
//
// The record is placed by the FORWARD placed record: read_end / ref_end are its, begin = end - non-gap bases, the score is the
// returned alignment re-scored, and a pair whose forward score is 0 is an all-zero record without ops.  Every index taken from
// a record is clamped before it addresses anything: idx[0] / idx[1] to [0, AL - 1] (the rows' columns), and a forward score of
// 0 reads no column at all.  A wrong record gives a wrong answer, never an address outside the pair's rows.
// All stores are ordinary vector stores; byte loads, consecutive lanes on consecutive (descending) bytes, no LDS.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cigar_kernels.hip.h"
#include "span_kernels.hip.h"

namespace valign {

struct SpanCigarArgs {
    const uint8_t *rows;      // n * 2 * AL: the child walk's result rows (reversed frame) of these pairs
    const short *idx;         // n * 4, the child's
    const PlacedRec *fwd;     // n forward placed records
    CigarRec *recs;           // n records, or null: ops only (the emit pass of the host path)
    unsigned *ops;            // or null: records only (the count pass of the host path)
    const long long *offsets; // not null: pair p's ops start at ops[offsets[p]] and all of them are stored;
    int ops_stride;           // null: at ops[p * ops_stride], the first min(n_ops, ops_stride) of them
    const CigarRec *recs_in;  // not null (emit pass): the records of the count pass, copied to recs_out behind the same launch
    CigarRec *recs_out;
    long long n;
    int AL;                   // of the child: read_length + span_ref_length
    int R, F;                 // of the forward pair: what read_end / ref_end are clamped to
    int extended;
    int affine;
    int match, mismatch, gap_read, gap_ref, open_read, ext_read, open_ref, ext_ref;
};

template <int W>
__global__ void __launch_bounds__(256)
span_cigar_encode_kernel(const SpanCigarArgs a) {
    static_assert(W == 16 || W == 64, "a quarter wave or a wave per pair");
    constexpr int kGroups = 256 / W;
    const int lane = threadIdx.x & (kWave - 1), l = lane & (W - 1), gbase = lane - l;
    const long long pair = (long long)blockIdx.x * kGroups + threadIdx.x / W;
    const bool live = pair < a.n;
    int start = 0, end = 0;
    PlacedRec f{0, 0, 0};
    if (live) {
        f = a.fwd[pair];
        start = (int)(unsigned short)a.idx[pair * 4 + 0];
        end = (int)(unsigned short)a.idx[pair * 4 + 1];
        if (end > a.AL - 1) end = a.AL - 1;                 // (never: the walk writes AL - 1; the rows end there)
        if (start > end) start = end;
        if (f.score <= 0) start = end;                      // an empty pair: zeros, whatever the child's rows hold
    }
    const int cols = end - start;
    // the groups of a wave step together (the ballot is the wave's): as many steps as the longest of them needs
    int steps = (cols + W - 1) / W;
    if constexpr (W < 64) {
#pragma unroll
        for (int d = W; d < kWave; d <<= 1) {
            const int other = __shfl_xor(steps, d, kWave);
            steps = other > steps ? other : steps;
        }
    }
    const uint8_t *row_read = a.rows + (live ? pair : 0) * 2 * a.AL, *row_ref = row_read + a.AL;
    unsigned *ops = nullptr;
    unsigned cap = 0;
    if (live && a.ops) {
        ops = a.offsets ? a.ops + a.offsets[pair] : a.ops + pair * a.ops_stride;
        cap = a.offsets ? 0xFFFFFFFFu : (unsigned)a.ops_stride;
    }
    unsigned count = 0;                    // runs begun so far (group-uniform)
    int carry_op = -1, carry_len = 0;      // the run still open at the end of the last step; its index is count - 1
    int read_bases = 0, ref_bases = 0, score = 0;
    for (int s = 0; s < steps; ++s) {
        const int k = s * W + l;           // the column's place in forward reading order
        const bool valid = k < cols;
        const int c = end - 1 - k;         // valid: start <= c <= end - 1 < AL - 1
        unsigned ca = 0, cb = 0;
        if (valid) {
            ca = row_read[c];
            cb = row_ref[c];
        }
        int op = -2;
        if (valid) {
            if (ca == '-' && cb != '-') op = kCigarD;
            else if (cb == '-' && ca != '-') op = kCigarI;
            else if (!a.extended) op = kCigarM;
            else op = ((ca | 0x20u) == (cb | 0x20u)) ? kCigarEq : kCigarX;
        }
        int prev = __shfl_up(op, 1, W);
        if (l == 0) prev = carry_op;
        const bool boundary = valid && op != prev;
        const unsigned long long gm = cigar_group_bits<W>(__ballot(boundary), gbase);
        const unsigned long long vm = cigar_group_bits<W>(__ballot(valid), gbase);
        const int nvalid = __popcll(vm);
        read_bases += __popcll(cigar_group_bits<W>(__ballot(valid && ca != '-'), gbase));
        ref_bases += __popcll(cigar_group_bits<W>(__ballot(valid && cb != '-'), gbase));
        if (valid && a.recs) {
            if (op == kCigarD) score += a.affine ? (prev == kCigarD ? a.ext_read : a.open_read) : a.gap_read;
            else if (op == kCigarI) score += a.affine ? (prev == kCigarI ? a.ext_ref : a.open_ref) : a.gap_ref;
            else {
                const int ka = base_class(ca), kb = base_class(cb);
                if (ka >= 1 && ka <= 4 && kb >= 1 && kb <= 4) score += ka == kb ? a.match : a.mismatch;
            }
        }
        // the carried run goes on for `first` columns of this step, and is closed by the step's first boundary
        const int first = gm ? __ffsll((long long)gm) - 1 : nvalid;
        if (carry_len > 0) {
            carry_len += first;
            if (gm && l == 0 && ops && count - 1 < cap) ops[count - 1] = ((unsigned)carry_len << 4) | (unsigned)carry_op;
        }
        if (boundary) {
            const unsigned long long above = l == 63 ? 0ull : gm >> (l + 1);
            const unsigned at = count + (unsigned)__popcll(gm & ((1ull << l) - 1ull));
            if (above && ops && at < cap) ops[at] = ((unsigned)__ffsll((long long)above) << 4) | (unsigned)op;     // closed inside the step
        }
        const int last = gm ? 63 - __clzll((long long)gm) : 0;       // the step's last boundary opens the run that is carried on
        const int last_op = __shfl(op, last, W);                     // (every lane of the wave takes part)
        if (gm) {
            carry_len = nvalid - last;
            carry_op = last_op;
            count += (unsigned)__popcll(gm);
        }
    }
    if (carry_len > 0 && l == 0 && ops && count - 1 < cap) ops[count - 1] = ((unsigned)carry_len << 4) | (unsigned)carry_op;
    if (a.recs) {
#pragma unroll
        for (int d = W / 2; d >= 1; d >>= 1) score += __shfl_xor(score, d, W);
        if (live && l == 0) {
            CigarRec r{0, 0, 0, 0, 0, 0u};
            if (cols > 0) {                    // (an empty pair -- forward score 0 -- is all zeros)
                r.read_end = span_clamp(f.read_end, a.R);
                r.ref_end = span_clamp(f.ref_end, a.F);
                r.read_begin = r.read_end - read_bases;
                r.ref_begin = r.ref_end - ref_bases;
                r.score = score;
                r.n_ops = count;
            }
            a.recs[pair] = r;
        }
    }
    if (a.recs_in && live && l < 6)            // emit pass: the record joins its ops in the buffer that crosses PCIe
        reinterpret_cast<unsigned *>(a.recs_out + pair)[l] = reinterpret_cast<const unsigned *>(a.recs_in + pair)[l];
}

}  // namespace valign
