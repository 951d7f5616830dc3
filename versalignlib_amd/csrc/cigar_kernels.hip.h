// cigar_kernels.hip.h -- gfx950 kernels of the compact result format (include/valign_hip.h: valign_hip_aln + 32-bit ops).
//
// The encoder sits BEHIND the traceback: it reads the two finished result rows of a pair in device memory (columns readStart ..
// readEnd - 1, idx[0] / idx[1] as the walk left them) and the pair's end cell, and writes one 24-byte record and the run-length
// encoded ops.  Every alignment route (fused, register geometries, row strips, strip_wide, strip_band, strip_ckpt, both tie-break
// policies) therefore feeds it without a change to a walk.  Column rule and run lengths are exactly vh_cigar's
// (valign_host.cpp): '-' in the read row only is D, '-' in the ref row only is I, else M -- or, extended, '=' where the two
// bytes are equal ignoring case and X where not.  vh_cigar_ops is the same statement on the CPU.
//
// Shape: a lane group of W lanes (16 or 64) per pair, consecutive lanes on consecutive columns, W columns per step.  Each lane
// classifies its column; the ballot of "op differs from the previous column" (the previous step's last op carried in) marks the
// run boundaries.  A boundary lane's run index is the popcount of the boundaries below it plus the runs before this step, its
// length the distance to the next boundary; the run that is still open at the end of a step is carried group-uniformly
// (op, length, index) and stored when a later step closes it.  Non-gap bases and the score are popcounts / a group reduction.
// All stores are ordinary vector stores.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trace_kernels.hip.h"

namespace valign {

constexpr int kCigarM = 0, kCigarI = 1, kCigarD = 2, kCigarEq = 7, kCigarX = 8;

struct CigarRec {             // = valign_hip_aln
    int read_begin, read_end, ref_begin, ref_end, score;
    unsigned n_ops;
};
static_assert(sizeof(CigarRec) == 24, "valign_hip_aln is 24 bytes");

struct CigarArgs {
    const uint8_t *rows;      // n * 2 * AL: the walk's result rows of these pairs
    const short *idx;         // n * 4
    const EndCell *ends;      // n end cells (records only; may be null when recs is)
    CigarRec *recs;           // n records, or null: ops only (the emit pass of the host path)
    unsigned *ops;            // or null: records only (the count pass of the host path)
    const long long *offsets; // not null: pair p's ops start at ops[offsets[p]] and all of them are stored;
    int ops_stride;           // null: at ops[p * ops_stride], the first min(n_ops, ops_stride) of them
    const CigarRec *recs_in;  // not null (emit pass): the records of the count pass, copied to recs_out behind the same launch
    CigarRec *recs_out;
    long long n;
    int AL;
    int extended;
    int affine;
    int match, mismatch, gap_read, gap_ref, open_read, ext_read, open_ref, ext_ref;
};

template <int W>
__device__ __forceinline__ unsigned long long cigar_group_bits(unsigned long long wave_mask, int gbase) {
    if constexpr (W == 64) return wave_mask;
    else return (wave_mask >> gbase) & ((1ull << W) - 1ull);
}

template <int W>
__global__ void __launch_bounds__(256)
cigar_encode_kernel(const CigarArgs a) {
    static_assert(W == 16 || W == 64, "a quarter wave or a wave per pair");
    constexpr int kGroups = 256 / W;
    const int lane = threadIdx.x & (kWave - 1), l = lane & (W - 1), gbase = lane - l;
    const long long pair = (long long)blockIdx.x * kGroups + threadIdx.x / W;
    const bool live = pair < a.n;
    int start = 0, end = 0;
    if (live) {
        start = (int)(unsigned short)a.idx[pair * 4 + 0];
        end = (int)(unsigned short)a.idx[pair * 4 + 1];
        if (end > a.AL - 1) end = a.AL - 1;                 // (never: the walk writes AL - 1; the rows end there)
        if (start > end) start = end;
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
        const int c = start + s * W + l;
        const bool valid = c < end;
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
            if (cols > 0) {                    // (an empty alignment -- SW maximum 0, an NW read that starts invalid -- is all zeros)
                const EndCell e = a.ends[pair];
                r.read_end = (int)e.read_pos + 1;
                r.ref_end = (int)e.ref_pos + 1;
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

#ifdef VALIGN_TU_CIGAR      // not a template: defined once, in engine_cigar.hip
// offsets[0 .. n] = exclusive scan of recs[p].n_ops (one block: a chunk of the host path is some ten thousand pairs)
__global__ void __launch_bounds__(1024)
cigar_scan_kernel(const CigarRec *recs, long long *offsets, long long n) {
    __shared__ long long wave_sum[16];
    __shared__ long long base;
    const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    if (t == 0) base = 0;
    __syncthreads();
    for (long long at = 0; at < n; at += 1024) {
        const long long p = at + t;
        const long long v = p < n ? (long long)recs[p].n_ops : 0;
        long long incl = v;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const long long other = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += other;
        }
        if (lane == kWave - 1) wave_sum[wave] = incl;
        __syncthreads();
        long long before = base;
        for (int w = 0; w < wave; ++w) before += wave_sum[w];
        if (p < n) offsets[p] = before + incl - v;
        __syncthreads();
        if (t == 1023) base = before + incl;
        __syncthreads();
    }
    if (t == 0) offsets[n] = base;
}
#endif

}  // namespace valign
