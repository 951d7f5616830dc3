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

// The record of an end cell: half-open 0-based ends, zeros for the empty alignment
__device__ __forceinline__ PlacedRec placed_record(const EndCell e) {
    PlacedRec r;
    const bool hit = e.score > 0;
    r.score = hit ? (int)e.score : 0;
    r.read_end = hit ? (int)e.read_pos + 1 : 0;
    r.ref_end = hit ? (int)e.ref_pos + 1 : 0;
    return r;
}

template <int G, int K, int GAPS, int TRACK>
__global__ void __launch_bounds__(256)
score_placed_kernel(const PlacedArgs args) {
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
        merge_profile<K>(pa, pb, S);                                     // step t's scores
        lds_load_lane<K>(lane_base + ca_next * geo::kPairStride, pa);     // step t+1's profile rows
        lds_load_lane<K>(lane_base + cb_next * geo::kPairStride, pb);
        ca_next = *(lds_cu8 *)(code_addr + 4);                            // step t+2's slab numbers
        cb_next = *(lds_cu8 *)(code_addr + 5);
        if (!MASKED || (unsigned)j < (unsigned)F) {
            const s16x2 tt = pk((short)t);
            s16x2 step_key = pk(0);
            // end-cell bookkeeping of one finished cell (SW cells are >= 0: rb - h cannot wrap)
            auto track = [&](int q, s16x2 hq) __attribute__((always_inline)) {
                if (KEY) {
                    step_key = pk_max(step_key, pk_mad_u(hq, key_mul, row_key[q]));
                } else {
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

}  // namespace valign
