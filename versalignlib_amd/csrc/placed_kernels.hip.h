// placed_kernels.hip.h -- placed Smith-Waterman scores (valign_hip_score_placed_*): the score of a pair AND the cell its best
// local alignment ends in, from the score sweep alone -- no codes, no pointer stream, no tags, no scratch.
//
// The end cell is the reference's (src/Kernels/default/DefaultKernel.cpp:252-256): the first cell in row-major order whose
// value is strictly greater than every earlier one, i.e. of all cells that hold the maximum the one in the earliest row and,
// within it, the earliest column.  score_placed_kernel is score_kernel's int16 Smith-Waterman sweep (dp_kernels.hip.h: same
// lane groups, query profile, LDS fetch one step ahead, two steps per trip, DPP moves in every lane before any select) with
// the end-cell tracking of the alignment fill kernels (trace_kernels.hip.h) in place of the bare maximum:
//   kPlacedKey:  one key per lane, value << BITS | (2^BITS - 1 - row of the lane), and the step at which it last grew: a
//                multiply-add and a maximum per register, four instructions per step.  BITS = placed_key_bits(K); the
//                rule (placed_choice, cell_rules.h) takes it where the largest possible value keeps the key inside int16.
//   kPlacedRows: a first-arg-max per row (value and step, four packed instructions per register): any K, any int16 score.
// Both track the finished cell h off the dependency chain: the bookkeeping of row q - 1 sits between the links of row q.
// write_end_cells (trace_kernels.hip.h) combines the lanes into the wave's LDS table; the group leader turns its two end
// cells into records with plain vector stores.
// The SUB form of the same kernel (suboptimal scores, valign_hip_score_subopt_*) also sends every column's maximum out of the
// wave; see SuboptArgs below and subopt_kernels.hip.h.
#pragma once

#include "cell_rules.h"
#include "trace_kernels.hip.h"

namespace valign {

struct PlacedRec {            // = valign_hip_placed (include/valign_hip.h), 12 bytes
    int score, read_end, ref_end;
};

struct PlacedArgs {
    const uint8_t *reads;     // n * R bytes, pair-major
    const uint8_t *refs;      // n * F bytes, pair-major
    PlacedRec *placed;        // n
    long long n;
    int R, F;
    int prof_area, refc_stride, wave_lds;
    short match, mismatch;
    short gap_read, gap_ref;
    short open_read, ext_read, open_ref, ext_ref;
};

constexpr int kPlacedKey = 0, kPlacedRows = 1;

// What the suboptimal-score form of the sweep (valign_hip_score_subopt_*; engine_subopt.hip) adds to a placed launch: where the
// column maxima go.  Lane G - 1 of a group puts every finished column into the group's ring in LDS; each time the ring is full
// (and after the last column) the whole wave flushes the rings of its groups, 16 bytes per lane.
struct SuboptArgs : PlacedArgs {
    unsigned *colmax;         // one row of col_stride dwords per pair of pairs: colmax[j] of pair A (low half) and pair B (high half)
    int col_stride;           // dwords, a multiple of 4: flushes are whole, aligned 16-byte stores
    int ring_ofs;             // bytes from the wave's LDS to its rings (16-byte aligned): kSuboptRingBytes behind the placed tables
};
constexpr int kSuboptRingBytes = 1024;                                  // per wave: 64 lanes x 16 bytes, one flush
constexpr int subopt_ring_cols(int G) { return kSuboptRingBytes / 4 / (kWave / G); }      // columns of a group's ring: 4 G, a power of two
typedef __attribute__((address_space(3))) unsigned lds_u32;

// The record of an end cell: half-open 0-based ends, zeros for the empty alignment
__device__ __forceinline__ PlacedRec placed_record(const EndCell e) {
    PlacedRec r;
    const bool hit = e.score > 0;
    r.score = hit ? (int)e.score : 0;
    r.read_end = hit ? (int)e.read_pos + 1 : 0;
    r.ref_end = hit ? (int)e.ref_pos + 1 : 0;
    return r;
}

// SUB: the suboptimal-score form (its launches take SuboptArgs).  Every addition sits behind `if constexpr (SUB)`: the sweep
// loops of the placed instances (SUB false) keep their instructions (DESIGN.md has the comparison against the assembly before).
template <int G, int K, int GAPS, int TRACK, bool SUB = false>
__global__ void __launch_bounds__(256)
score_placed_kernel(const std::conditional_t<SUB, SuboptArgs, PlacedArgs> args) {
    static_assert(GAPS == kGapLinear || GAPS == kGapSym || GAPS == kGapAffine || GAPS == kGapAffineSym, "placed scores run on int16 cells");
    static_assert(TRACK == kPlacedRows || K <= kPlacedKeyMaxK, "the lane key exists for up to 16 rows per lane");
    using geo = Geo<G, K>;
    constexpr bool AFFINE = GAPS == kGapAffine || GAPS == kGapAffineSym;
    constexpr bool SYM = GAPS == kGapSym;
    constexpr bool AFFSYM = GAPS == kGapAffineSym;
    constexpr bool KEY = TRACK == kPlacedKey;
    constexpr int kKeyBits = placed_key_bits(K);
    const int lane = threadIdx.x & (kWave - 1);
    const int grp = lane / G;
    const int l = lane % G;
    const int pad_rows = geo::kRows - args.R;

    WaveTables w;
    if (!wave_setup<G, K, false>(args.reads, args.refs, args.n, args.R, args.F, args.prof_area, args.refc_stride, args.wave_lds,
                                 args.match, args.mismatch, w))
        return;
    // columns after the last ACGT base of every reference in the wave score nothing: no cell there is STRICTLY greater
    const int F = w.cols_used;

    const unsigned lmask = l == 0 ? 0u : 0xFFFFFFFFu;
    const unsigned lane_base = lds_offset(w.prof) + l * geo::kLaneBytes;
    unsigned code_addr = lds_offset(w.refc) + grp * args.refc_stride - 2 * l;

    // magnitudes for the unsigned floor-at-zero subtract
    const s16x2 g_read = pk((short)-args.gap_read), g_ref = pk((short)-args.gap_ref);
    const s16x2 o_read = pk((short)-args.open_read), e_read = pk((short)-args.ext_read);
    const s16x2 o_ref = pk((short)-args.open_ref), e_ref = pk((short)-args.ext_ref);
    // constants of the packed key / arg-max arithmetic stay in VGPRs the optimiser cannot see through (align_fill_kernel)
    s16x2 fifteen = pk(15), key_mul = pk((short)(1 << kKeyBits));
    asm volatile("" : "+v"(fifteen), "+v"(key_mul));

    constexpr int kTracked = KEY ? 1 : K;
    s16x2 Hl[K], El[AFFINE ? K : 1], HOl[AFFSYM ? K : 1];
    s16x2 rb[kTracked], fc[kTracked];
    s16x2 row_key[KEY ? K : 1];                  // 2^BITS - 1 - q: the earlier row wins among equal values
#pragma unroll
    for (int q = 0; q < K; ++q) {
        Hl[q] = pk(0);
        if (AFFINE) El[q] = pk(0);
        if (AFFSYM) HOl[q] = pk(0);
        if (KEY) {
            row_key[q] = pk((short)((1 << kKeyBits) - 1 - q));
            asm volatile("" : "+v"(row_key[q]));
        } else {
            rb[q] = pk(0);
            fc[q] = pk(0);
        }
    }
    if (KEY) rb[0] = fc[0] = pk(0);
    s16x2 up0 = pk(0), h_last = pk(0), f_last = pk(0);
    int j = -l;

    // Suboptimal scores: the column's maximum over the rows below each pair's trimmed read length travels from lane to lane
    // beside h_last -- lane G - 1 holds column t - (G - 1) complete at step t.  Rows at or beyond the trimmed length do not
    // count: the key track multiplies them by 0 instead of 2^BITS (their keys then carry the value 0; the placed record keeps
    // its cell, which no such row ever holds -- they only repeat values down the diagonals), the rows track ANDs a mask.
    // (The geometry's pad rows lie on top and hold zeros.)
    constexpr int kRing = subopt_ring_cols(G);
    s16x2 row_mul[SUB && KEY ? K : 1], row_keep[SUB && !KEY ? K : 1];
    s16x2 cm_last = pk(0);
    unsigned ring_lds = 0;
    if constexpr (SUB) {
        int trimmed[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            int p = 2 * grp + half;
            p = p > w.last ? w.last : p;
            const uint8_t *rd = args.reads + (w.pair0 + p) * args.R;
            int len = 0;
            for (int pos = l; pos < args.R; pos += G) {
                const int c = base_class(rd[pos]);
                if (c >= 1 && c <= 4) len = pos + 1;
            }
#pragma unroll
            for (int dd = G / 2; dd >= 1; dd >>= 1) {
                const int other = __shfl_xor(len, dd, kWave);
                len = other > len ? other : len;
            }
            trimmed[half] = len;
        }
#pragma unroll
        for (int q = 0; q < K; ++q) {
            const int pos = l * K + q - pad_rows;
            const bool in_a = pos < trimmed[0], in_b = pos < trimmed[1];
            if constexpr (KEY) {
                row_mul[q] = s16x2{(short)(in_a ? 1 << kKeyBits : 0), (short)(in_b ? 1 << kKeyBits : 0)};
                asm volatile("" : "+v"(row_mul[q]));
            } else {
                row_keep[q] = s16x2{(short)(in_a ? -1 : 0), (short)(in_b ? -1 : 0)};
            }
        }
        ring_lds = lds_offset(w.prof) + args.ring_ofs;
    }
    // the wave's rings -> the rows of its pairs of pairs, columns [base, base + kRing): lane i moves dwords 4 i .. 4 i + 3
    auto flush = [&](int base) __attribute__((always_inline)) {
        if constexpr (SUB) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int g = (4 * lane) / kRing, c = base + (4 * lane) % kRing;
            const u32x4 v = *(lds_cu32x4 *)(ring_lds + 16 * lane);
            const long long pp = w.pair0 / 2 + g;
            if (2 * pp < args.n && c < args.col_stride) *reinterpret_cast<u32x4 *>(args.colmax + (size_t)pp * args.col_stride + c) = v;
            __builtin_amdgcn_wave_barrier();
        }
    };

    // LDS fetches run one step ahead of the arithmetic, as in score_kernel
    unsigned pa[K / 2], pb[K / 2];
    s16x2 S0[K], S1[K];
    unsigned ca_next, cb_next;
    {
        const unsigned ca = *(lds_cu8 *)(code_addr), cb = *(lds_cu8 *)(code_addr + 1);
        lds_load_lane<K>(lane_base + ca * geo::kPairStride, pa);
        lds_load_lane<K>(lane_base + cb * geo::kPairStride, pb);
        ca_next = *(lds_cu8 *)(code_addr + 2);
        cb_next = *(lds_cu8 *)(code_addr + 3);
    }

    auto step = [&](auto masked_tag, int t, s16x2 (&S)[K]) __attribute__((always_inline)) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        const s16x2 diag0 = up0;
        // every lane takes part in the DPP moves, before the select on the lane's column
        up0 = as_pk(group_prev_or_zero<G>(as_u32(h_last), lmask));
        s16x2 fup0 = pk(0);
        if (AFFINE) fup0 = as_pk(group_prev_or_zero<G>(as_u32(f_last), lmask));
        s16x2 cm_in = pk(0);
        if constexpr (SUB) cm_in = as_pk(group_prev_or_zero<G>(as_u32(cm_last), lmask));      // this column, as far as the lanes before have it
        merge_profile<K>(pa, pb, S);                                     // step t's scores
        lds_load_lane<K>(lane_base + ca_next * geo::kPairStride, pa);     // step t+1's profile rows
        lds_load_lane<K>(lane_base + cb_next * geo::kPairStride, pb);
        ca_next = *(lds_cu8 *)(code_addr + 4);                            // step t+2's slab numbers
        cb_next = *(lds_cu8 *)(code_addr + 5);
        if (!MASKED || (unsigned)j < (unsigned)F) {
            const s16x2 tt = pk((short)t);
            s16x2 step_key = pk(0);
            s16x2 col_own = pk(0);                                       // SUB, rows track: the maximum of the lane's counted rows
            // end-cell bookkeeping of one finished cell (SW cells are >= 0: rb - h cannot wrap)
            auto track = [&](int q, s16x2 hq) __attribute__((always_inline)) {
                if (KEY) {
                    if constexpr (SUB) step_key = pk_max(step_key, pk_mad_u(hq, row_mul[q], row_key[q]));
                    else step_key = pk_max(step_key, pk_mad_u(hq, key_mul, row_key[q]));
                } else {
                    if constexpr (SUB) col_own = pk_max(col_own, as_pk(as_u32(hq) & as_u32(row_keep[q])));
                    const s16x2 changed = (rb[q] - hq) >> fifteen;       // 0xFFFF where h beats the row's best: the first column is kept
                    fc[q] = as_pk((as_u32(changed) & as_u32(tt)) | (~as_u32(changed) & as_u32(fc[q])));
                    rb[q] = pk_max(rb[q], hq);
                }
            };
            s16x2 h_prev = pk(0);
            if (SYM) {
                // h = max(diag + S, max(left, up) - g): score_kernel's chain, the next row's diag + S and the previous row's
                // bookkeeping written between its links
                s16x2 h = up0;
                s16x2 d_cur = diag0 + S[0];
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    const s16x2 x = pk_max(Hl[q], h);
                    s16x2 d_next = pk(0);
                    if (q + 1 < K) d_next = Hl[q] + S[q + 1];
                    const s16x2 y = pk_sub_floor0(x, g_ref);
                    if (q > 0) track(q - 1, h_prev);
                    h = pk_max(d_cur, y);
                    Hl[q] = h;
                    h_prev = h;
                    d_cur = d_next;
                }
                track(K - 1, h_prev);
                h_last = h;
            } else {
                // pass1(q): what row q needs of the previous column only, one row ahead of the chain down the column
                auto pass1 = [&](int q) __attribute__((always_inline)) -> s16x2 {
                    const s16x2 d = (q == 0 ? diag0 : Hl[q - 1]) + S[q];
                    s16x2 e;
                    if (AFFSYM) {
                        e = pk_max(pk_sub_floor0(El[q], e_read), HOl[q]);
                        El[q] = e;
                    } else if (AFFINE) {
                        e = pk_max(pk_sub_floor0(El[q], e_read), pk_sub_floor0(Hl[q], o_read));
                        El[q] = e;
                    } else {
                        e = pk_sub_floor0(Hl[q], g_read);
                    }
                    return pk_max(d, e);
                };
                s16x2 h = up0, f = fup0;
                s16x2 ho = pk(0);
                if (AFFSYM) ho = pk_sub_floor0(up0, o_ref);
                s16x2 m_cur = pass1(0);
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    if (AFFSYM) f = pk_max(pk_sub_floor0(f, e_ref), ho);
                    else if (AFFINE) f = pk_max(pk_sub_floor0(f, e_ref), pk_sub_floor0(h, o_ref));
                    else f = pk_sub_floor0(h, g_ref);
                    s16x2 m_next = pk(0);
                    if (q + 1 < K) m_next = pass1(q + 1);        // before Hl[q] is overwritten
                    if (q > 0) track(q - 1, h_prev);
                    h = pk_max(m_cur, f);
                    Hl[q] = h;
                    if (AFFSYM) {
                        ho = pk_sub_floor0(h, o_ref);
                        HOl[q] = ho;
                    }
                    h_prev = h;
                    m_cur = m_next;
                }
                track(K - 1, h_prev);
                h_last = h;
                f_last = f;
            }
            if (KEY) {
                const s16x2 changed = (rb[0] - step_key) >> fifteen;      // keys are >= 0: no wrap
                fc[0] = as_pk((as_u32(changed) & as_u32(tt)) | (~as_u32(changed) & as_u32(fc[0])));
                rb[0] = pk_max(rb[0], step_key);
            }
            if constexpr (SUB) {
                // keys travel as they are (the larger key holds the larger value); lane G - 1 drops the row bits
                cm_last = pk_max(cm_in, KEY ? step_key : col_own);
                if (l == G - 1) {
                    const s16x2 done = KEY ? (s16x2)((u16x2)cm_last >> (unsigned short)kKeyBits) : cm_last;
                    *(lds_u32 *)(ring_lds + (grp * kRing + (j & (kRing - 1))) * 4) = as_u32(done);
                }
            }
        }
        if constexpr (SUB) {
            const int col = t - (G - 1);                                  // wave-uniform: the column the last lanes just finished
            if (col >= 0 && (((col + 1) & (kRing - 1)) == 0 || col == F - 1)) flush(col & ~(kRing - 1));
        }
        ++j;
        code_addr += 2;
    };

    const int steps = F + G - 1;
    const int fill_end = G - 1 < steps ? G - 1 : steps;
    const int steady_end = F > fill_end ? F : fill_end;
    int t = 0;
    for (; t < fill_end; ++t) step(std::true_type{}, t, S0);
    for (; t + 1 < steady_end; t += 2) {       // two steps per trip: loop-carried registers swap roles
        step(std::false_type{}, t, S0);
        step(std::false_type{}, t + 1, S1);
    }
    for (; t < steady_end; ++t) step(std::false_type{}, t, S0);
    for (; t < steps; ++t) step(std::true_type{}, t, S0);

    // ---- the lanes' end cells combined (write_end_cells: into the wave's LDS table), then one record per pair ----
    FillArgs fa{};
    fa.n = args.n;
    EndCell *wave_ends = reinterpret_cast<EndCell *>(w.first_bad);      // kPairs x 8 bytes behind the wave's tables, unused by this sweep
    const int none[2] = {0, 0};
    if constexpr (KEY) write_end_cells<G, K, kAlgSW, kKeyBits>(fa, w, rb, fc, none, none, pad_rows, lane, grp, l, 0, wave_ends);
    else write_end_cells<G, K, kAlgSW>(fa, w, rb, fc, none, none, pad_rows, lane, grp, l, 0, wave_ends);
    if (l == 0) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const long long pair = w.pair0 + 2 * grp + half;
            if (pair < args.n) args.placed[pair] = placed_record(wave_ends[2 * grp + half]);      // (this lane wrote the entry)
        }
    }
}

#ifdef VALIGN_TU_PLACED      // not a template: defined once, in engine_placed.hip
// The strip path's end cells (align_strip_kernel merges them strip after strip) -> records
__global__ void __launch_bounds__(256)
placed_records_kernel(const EndCell *ends, PlacedRec *placed, long long n) {
    const long long pair = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pair < n) placed[pair] = placed_record(ends[pair]);
}
#endif

// The instances: the two symmetric gap forms with the lane key on every geometry of up to 16 rows per lane; the two asymmetric
// forms with the key and all four forms per row on the full geometries (and per row on 64 x 24, which has no key form) -- a
// call that needs one of these on another geometry is re-planned onto the next full one, as alignments are.
// placed_kernel<G, K, FULL>(track, gap form): the instance, or nullptr where none is compiled for the geometry.  The engine
// units see the declaration only; the kernel parts (kernel_part.hip) define and instantiate it, and with it the kernels.
template <int G, int K, bool FULL>
const void *placed_kernel(int track, int gaps);

#ifdef VALIGN_KERNEL_PART_TU
template <int G, int K, bool FULL>
const void *placed_kernel(int track, int gaps) {
    const void *placed[2][4] = {};
    if constexpr (K <= kPlacedKeyMaxK) {
        placed[kPlacedKey][kGapSym] = (const void *)&score_placed_kernel<G, K, kGapSym, kPlacedKey>;
        placed[kPlacedKey][kGapAffineSym] = (const void *)&score_placed_kernel<G, K, kGapAffineSym, kPlacedKey>;
        if constexpr (FULL) {
            placed[kPlacedKey][kGapLinear] = (const void *)&score_placed_kernel<G, K, kGapLinear, kPlacedKey>;
            placed[kPlacedKey][kGapAffine] = (const void *)&score_placed_kernel<G, K, kGapAffine, kPlacedKey>;
        }
    }
    if constexpr (FULL || (G == 64 && K == 24)) {
        placed[kPlacedRows][kGapLinear] = (const void *)&score_placed_kernel<G, K, kGapLinear, kPlacedRows>;
        placed[kPlacedRows][kGapSym] = (const void *)&score_placed_kernel<G, K, kGapSym, kPlacedRows>;
        placed[kPlacedRows][kGapAffine] = (const void *)&score_placed_kernel<G, K, kGapAffine, kPlacedRows>;
        placed[kPlacedRows][kGapAffineSym] = (const void *)&score_placed_kernel<G, K, kGapAffineSym, kPlacedRows>;
    }
    return (track == kPlacedKey || track == kPlacedRows) && gaps >= 0 && gaps < 4 ? placed[track][gaps] : nullptr;
}
#endif

// The suboptimal-score instances, on the six full geometries only: the key track where K <= 16, the rows track on all six, the
// four gap forms each (5 x 4 + 6 x 4 = 44 instances).  A call whose plan is another geometry is re-planned onto the next full one.
template <int G, int K, bool FULL>
const void *subopt_kernel(int track, int gaps);

#ifdef VALIGN_KERNEL_PART_TU
template <int G, int K, bool FULL>
const void *subopt_kernel(int track, int gaps) {
    const void *sub[2][4] = {};
    if constexpr (FULL) {
        if constexpr (K <= kPlacedKeyMaxK) {
            sub[kPlacedKey][kGapLinear] = (const void *)&score_placed_kernel<G, K, kGapLinear, kPlacedKey, true>;
            sub[kPlacedKey][kGapSym] = (const void *)&score_placed_kernel<G, K, kGapSym, kPlacedKey, true>;
            sub[kPlacedKey][kGapAffine] = (const void *)&score_placed_kernel<G, K, kGapAffine, kPlacedKey, true>;
            sub[kPlacedKey][kGapAffineSym] = (const void *)&score_placed_kernel<G, K, kGapAffineSym, kPlacedKey, true>;
        }
        sub[kPlacedRows][kGapLinear] = (const void *)&score_placed_kernel<G, K, kGapLinear, kPlacedRows, true>;
        sub[kPlacedRows][kGapSym] = (const void *)&score_placed_kernel<G, K, kGapSym, kPlacedRows, true>;
        sub[kPlacedRows][kGapAffine] = (const void *)&score_placed_kernel<G, K, kGapAffine, kPlacedRows, true>;
        sub[kPlacedRows][kGapAffineSym] = (const void *)&score_placed_kernel<G, K, kGapAffineSym, kPlacedRows, true>;
    }
    return (track == kPlacedKey || track == kPlacedRows) && gaps >= 0 && gaps < 4 ? sub[track][gaps] : nullptr;
}
#endif

}  // namespace valign
