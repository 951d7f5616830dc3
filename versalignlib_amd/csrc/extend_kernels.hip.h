// extend_kernels.hip.h -- extension scores (valign_hip_score_extend_*): the best score of an alignment that STARTS at the anchor,
// before read[0] and ref[0], and ends anywhere -- with the cell it ends in -- plus the best score that consumes the read to its
// last base (include/valign_hip.h has the definition; tests/extend_ref.py restates it in numpy).
//
// score_extend_kernel is a sibling of score_placed_kernel's rows track (placed_kernels.hip.h): the same lane groups, the query
// profile in LDS, the fetch one step ahead, two steps per trip, the DPP hand-over of h_last / f_last and a first arg-max per row.
// What differs is the matrix: gap-priced borders and no floor at zero, so signed saturating packed adds and signed maxima stand
// where the placed sweep subtracts with a floor.
//
// The borders.  The read sits TOP-aligned in the lane tile (wave_setup's strip_row0 = 0): padded row p is read position p, the
// geometry's pad rows lie BELOW the read.  A pad row only reads what lies above it and nothing reads a pad row, so no condition
// falls on the pad rows' profile entries or border values, and wave_setup stays as it is.
//   * border column X(i, -1): the initial value of row i's Hl (the LEFT and the DIAG input of column 0), of up0 (the row above
//     the lane's first: its DIAG input of column 0), of h_last (what the lane behind receives while this lane has not started)
//     and of the row's running best, so that column -1 can win the row.  Affine: E starts at -32768, which loses every maximum
//     and stays there under the saturating add.  Pad rows take the value of row R - 1: inside the range the rule vouches for.
//   * border row X(-1, j): enters at lane 0 as the `up` input of step t -- one running add, OR-ed onto the zero the DPP move
//     leaves in a group's first lane; F of the border row is -32768 the same way.
// Tracking.  rb / fc hold each row's first arg-max over the columns j < Fp of ITS pair (the two halves of a register have
// different Fp: a packed column mask) -- the sign of the SATURATING rb - h decides, which cannot wrap whatever the two cells
// are.  The end cell of the best cell > 0 comes out of write_end_cells unchanged (a row or column of padding only repeats
// values down the diagonals, so the first cell that holds the maximum is a real one); gscore / gref_end are row Rp - 1's entry.
#pragma once

#include "cell_rules.h"
#include "extend_zdrop.h"
#include "trace_kernels.hip.h"

namespace valign {

struct ExtendRec {            // = valign_hip_extend (include/valign_hip.h), 20 bytes
    int score, read_end, ref_end, gscore, gref_end;
};

struct ExtendArgs {
    const uint8_t *reads;     // n * R bytes, pair-major
    const uint8_t *refs;      // n * F bytes, pair-major
    ExtendRec *extend;        // n
    long long n;
    int R, F;
    int prof_area, refc_stride, wave_lds;
    short match, mismatch;
    short gap_read, gap_ref;
    short open_read, ext_read, open_ref, ext_ref;
    int Z;                    // the ZDROP instances: extend_zdrop (> 0)
};

// a - b, saturating: the sign is that of the exact difference for any two int16 values
__device__ __forceinline__ s16x2 pk_sub_sat(s16x2 a, s16x2 b) { return __builtin_elementwise_sub_sat(a, b); }

// ZDROP (keys extend_zdrop > 0 and extend_zdrop_rows = 1; extend_zdrop.h has the rule, its lane form and why the minimum of the
// lanes' answers is the serial drop row): the record of one half of the packed registers, decided in the epilogue from rb / fc --
// the sweep itself does not change.  Every lane of the wave takes part (shuffles); every lane of the group returns the pair's
// record and T, the first dropping row, Rp where none drops.  Steps: unpack to (m, c = fc - l); the lane's combine; an inclusive
// scan over the group by __shfl_up, shifted by one lane and seeded with the anchor; the lane's replay; the minimum by an xor
// butterfly; the record from the lane that holds T (extend_zdrop_record_lane), which is also the lane of row Rp - 1 where T == Rp.
template <int G, int K>
__device__ __forceinline__ ExtendRec extend_zdrop_rows_record(const s16x2 (&rb)[K], const s16x2 (&fc)[K], int half, int lane, int l, int Rp, int Z,
                                                              int price_ref, int price_read, int &T_pair) {
    int m[K], c[K];
#pragma unroll
    for (int q = 0; q < K; ++q) {
        m[q] = half ? rb[q].y : rb[q].x;
        c[q] = (half ? fc[q].y : fc[q].x) - l;         // step -> column: the border column is -1
    }
    const int first_row = l * K;
    ExtendZdropBest run = extend_zdrop_lane_best(m, c, K, first_row, Rp);
#pragma unroll
    for (int dd = 1; dd < G; dd <<= 1) {
        const ExtendZdropBest before{__shfl_up(run.m, dd, kWave), __shfl_up(run.i, dd, kWave), __shfl_up(run.j, dd, kWave)};
        if (l >= dd) run = extend_zdrop_combine(before, run);
    }
    const ExtendZdropBest upto{__shfl_up(run.m, 1, kWave), __shfl_up(run.i, 1, kWave), __shfl_up(run.j, 1, kWave)};
    const ExtendZdropBest prefix = l == 0 ? extend_zdrop_anchor() : extend_zdrop_combine(extend_zdrop_anchor(), upto);
    const ExtendZdropLane mine = extend_zdrop_replay_lane(m, c, K, first_row, Rp, kExtendZdropNone, prefix, Z, price_ref, price_read);
    int T = mine.T;
#pragma unroll
    for (int dd = G / 2; dd >= 1; dd >>= 1) {
        const int other = __shfl_xor(T, dd, kWave);
        T = other < T ? other : T;
    }
    T = T < Rp ? T : Rp;
    // row Rp - 1's own entry, in the lane that holds it
    const int last_q = Rp > 0 ? (Rp - 1) % K : -1;
    int gs = 0, ge = 0;
#pragma unroll
    for (int q = 0; q < K; ++q) {
        if (q == last_q) {
            gs = m[q];
            ge = c[q] + 1;                              // half-open: the border column is 0
        }
    }
    const int src = lane - l + (Rp > 0 ? extend_zdrop_record_lane(T, Rp, K) : 0);
    ExtendRec rec;
    rec.score = __shfl(mine.best.m, src, kWave);
    rec.read_end = __shfl(mine.best.i, src, kWave) + 1;       // half-open ends; the anchor is three zeros
    rec.ref_end = __shfl(mine.best.j, src, kWave) + 1;
    rec.gscore = __shfl(gs, src, kWave);
    rec.gref_end = __shfl(ge, src, kWave);
    if (extend_zdrop_unreached(T, Rp)) {
        rec.gscore = kExtendZdropUnreached;
        rec.gref_end = 0;
    }
    T_pair = T;
    return rec;
}

template <int G, int K, int GAPS, bool ZDROP = false>
__global__ void __launch_bounds__(256)
score_extend_kernel(const ExtendArgs args) {
    static_assert(GAPS == kGapLinear || GAPS == kGapSym || GAPS == kGapAffine || GAPS == kGapAffineSym, "extension scores run on int16 cells");
    using geo = Geo<G, K>;
    constexpr bool AFFINE = GAPS == kGapAffine || GAPS == kGapAffineSym;
    constexpr bool SYM = GAPS == kGapSym;
    constexpr bool AFFSYM = GAPS == kGapAffineSym;
    constexpr short kLoses = -32768;
    const int lane = threadIdx.x & (kWave - 1);
    const int grp = lane / G;
    const int l = lane % G;
    const int R = args.R;

    WaveTables w;
    // strip_row0 = 0: padded row 0 is read position 0, rows at and beyond R are padding (class 0, score 0)
    if (!wave_setup<G, K, false>(args.reads, args.refs, args.n, R, args.F, args.prof_area, args.refc_stride, args.wave_lds,
                                 args.match, args.mismatch, w, false, blockIdx.x, 0, 0))
        return;
    // columns after the last ACGT base of every reference in the wave only repeat earlier values: never strictly greater, and
    // no candidate of any pair's gscore
    const int F = w.cols_used;

    // ---- trimmed lengths of the group's two pairs: 1 + the position of the last ACGT byte (the read's from HBM, the
    // reference's from the slab numbers wave_setup left: everything but ACGT took the zero slab) ----
    int Rp[2], Fp[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        int p = 2 * grp + half;
        p = p > w.last ? w.last : p;
        const uint8_t *rd = args.reads + (w.pair0 + p) * R;
        int rlen = 0, flen = 0;
        for (int pos = l; pos < R; pos += G) {
            const int c = base_class(rd[pos]);
            if (c >= 1 && c <= 4) rlen = pos + 1;
        }
        const unsigned codes = lds_offset(w.refc) + grp * args.refc_stride + half;
        for (int col = l; col < F; col += G)
            if (*(lds_cu8 *)(codes + 2 * col) != (unsigned)geo::kZeroSlab) flen = col + 1;
#pragma unroll
        for (int dd = G / 2; dd >= 1; dd >>= 1) {
            const int other_r = __shfl_xor(rlen, dd, kWave), other_f = __shfl_xor(flen, dd, kWave);
            rlen = other_r > rlen ? other_r : rlen;
            flen = other_f > flen ? other_f : flen;
        }
        Rp[half] = rlen;
        Fp[half] = flen;
    }
    const s16x2 fp = s16x2{(short)Fp[0], (short)Fp[1]};

    const unsigned lmask = l == 0 ? 0u : 0xFFFFFFFFu;
    const unsigned lane_base = lds_offset(w.prof) + l * geo::kLaneBytes;
    unsigned code_addr = lds_offset(w.refc) + grp * args.refc_stride - 2 * l;

    // the scores themselves, all <= 0: added with saturation
    const s16x2 g_read = pk(args.gap_read), g_ref = pk(args.gap_ref);
    const s16x2 o_read = pk(args.open_read), e_read = pk(args.ext_read);
    const s16x2 o_ref = pk(args.open_ref), e_ref = pk(args.ext_ref);
    s16x2 fifteen = pk(15);
    asm volatile("" : "+v"(fifteen));

    // X(i, -1): a gap of i + 1 read bases against nothing; X(-1, -1) = 0; pad rows as row R - 1
    auto border_col = [&](int row) __attribute__((always_inline)) -> short {
        const int i = row < R ? row : R - 1;
        if (i < 0) return 0;
        return (short)(AFFINE ? args.open_ref + i * args.ext_ref : (i + 1) * args.gap_ref);
    };

    s16x2 Hl[K], El[AFFINE ? K : 1], HOl[AFFSYM ? K : 1];
    s16x2 rb[K], fc[K];
#pragma unroll
    for (int q = 0; q < K; ++q) {
        Hl[q] = pk(border_col(l * K + q));
        if (AFFINE) El[q] = pk(kLoses);
        if (AFFSYM) HOl[q] = pk_add_sat(Hl[q], o_ref);
        rb[q] = Hl[q];                           // the row's best so far: column -1 ...
        fc[q] = pk((short)(l - 1));              // ... which this lane would sweep at step l - 1
    }
    s16x2 up0 = pk(border_col(l * K - 1)), h_last = pk(border_col(l * K + K - 1)), f_last = pk(kLoses);
    // the border row, in lane 0 only: X(-1, t) and what a step adds to it; F of the border row loses
    s16x2 lead_h = pk(0), lead_step = pk(0), lead_f = pk(0);
    if (l == 0) {
        lead_h = AFFINE ? o_read : g_read;
        lead_step = AFFINE ? e_read : g_read;
        lead_f = pk(kLoses);
    }
    int j = -l;

    // LDS fetches run one step ahead of the arithmetic, as in score_placed_kernel
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
        up0 = group_prev_or<G>(h_last, lead_h, lmask);
        lead_h = pk_add_sat(lead_h, lead_step);
        s16x2 fup0 = pk(0);
        if (AFFINE) fup0 = group_prev_or<G>(f_last, lead_f, lmask);
        merge_profile<K>(pa, pb, S);                                     // step t's scores
        lds_load_lane<K>(lane_base + ca_next * geo::kPairStride, pa);     // step t+1's profile rows
        lds_load_lane<K>(lane_base + cb_next * geo::kPairStride, pb);
        ca_next = *(lds_cu8 *)(code_addr + 4);                            // step t+2's slab numbers
        cb_next = *(lds_cu8 *)(code_addr + 5);
        if (!MASKED || (unsigned)j < (unsigned)F) {
            const s16x2 tt = pk((short)t);
            // 0xFFFF in the half whose pair still has column j below its trimmed reference length
            const s16x2 in_cols = pk_sub_sat(pk((short)j), fp) >> fifteen;
            // first arg-max of one finished cell (signed cells: the saturating difference keeps its sign)
            auto track = [&](int q, s16x2 hq) __attribute__((always_inline)) {
                const unsigned changed = as_u32(pk_sub_sat(rb[q], hq) >> fifteen) & as_u32(in_cols);      // 0xFFFF where h beats the row's best
                fc[q] = as_pk((changed & as_u32(tt)) | (~changed & as_u32(fc[q])));
                rb[q] = as_pk((changed & as_u32(hq)) | (~changed & as_u32(rb[q])));
            };
            s16x2 h_prev = pk(0);
            if (SYM) {
                // h = max(diag + S, max(left, up) + g): the next row's diag + S and the previous row's bookkeeping between the links
                s16x2 h = up0;
                s16x2 d_cur = pk_add_sat(diag0, S[0]);
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    const s16x2 x = pk_max(Hl[q], h);
                    s16x2 d_next = pk(0);
                    if (q + 1 < K) d_next = pk_add_sat(Hl[q], S[q + 1]);
                    const s16x2 y = pk_add_sat(x, g_ref);
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
                    const s16x2 d = pk_add_sat(q == 0 ? diag0 : Hl[q - 1], S[q]);
                    s16x2 e;
                    if (AFFSYM) {
                        e = pk_max(pk_add_sat(El[q], e_read), HOl[q]);
                        El[q] = e;
                    } else if (AFFINE) {
                        e = pk_max(pk_add_sat(El[q], e_read), pk_add_sat(Hl[q], o_read));
                        El[q] = e;
                    } else {
                        e = pk_add_sat(Hl[q], g_read);
                    }
                    return pk_max(d, e);
                };
                s16x2 h = up0, f = fup0;
                s16x2 ho = pk(0);
                if (AFFSYM) ho = pk_add_sat(up0, o_ref);
                s16x2 m_cur = pass1(0);
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    if (AFFSYM) f = pk_max(pk_add_sat(f, e_ref), ho);
                    else if (AFFINE) f = pk_max(pk_add_sat(f, e_ref), pk_add_sat(h, o_ref));
                    else f = pk_add_sat(h, g_ref);
                    s16x2 m_next = pk(0);
                    if (q + 1 < K) m_next = pass1(q + 1);        // before Hl[q] is overwritten
                    if (q > 0) track(q - 1, h_prev);
                    h = pk_max(m_cur, f);
                    Hl[q] = h;
                    if (AFFSYM) {
                        ho = pk_add_sat(h, o_ref);
                        HOl[q] = ho;
                    }
                    h_prev = h;
                    m_cur = m_next;
                }
                track(K - 1, h_prev);
                h_last = h;
                f_last = f;
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

    if constexpr (ZDROP) {
        // ---- the records under the rule: the group leader writes the five numbers the epilogue helper hands every lane ----
        const int price_ref = extend_zdrop_price(AFFINE ? args.ext_ref : args.gap_ref), price_read = extend_zdrop_price(AFFINE ? args.ext_read : args.gap_read);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            int T;
            const ExtendRec rec = extend_zdrop_rows_record<G, K>(rb, fc, half, lane, l, Rp[half], args.Z, price_ref, price_read, T);
            const long long pair = w.pair0 + 2 * grp + half;
            if (l == 0 && pair < args.n) args.extend[pair] = rec;
        }
        return;
    }
    // ---- the best cell > 0 of each pair (write_end_cells: into the wave's LDS table; no pad rows above the read) ----
    FillArgs fa{};
    fa.n = args.n;
    EndCell *wave_ends = reinterpret_cast<EndCell *>(w.first_bad);      // kPairs x 8 bytes behind the wave's tables, unused by this sweep
    const int none[2] = {0, 0};
    write_end_cells<G, K, kAlgSW>(fa, w, rb, fc, none, none, 0, lane, grp, l, 0, wave_ends);
    // ---- the records: the group leader writes the anchored score and its end cell, the lane that holds row Rp - 1 the
    // read-end score and its column (different dwords of the record; a read without a base is five zeros from the leader) ----
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const long long pair = w.pair0 + 2 * grp + half;
        if (pair >= args.n) continue;
        ExtendRec *rec = args.extend + pair;
        if (l == 0) {
            const EndCell e = wave_ends[2 * grp + half];                 // (this lane wrote the entry)
            const bool hit = e.score > 0;
            rec->score = hit ? (int)e.score : 0;
            rec->read_end = hit ? (int)e.read_pos + 1 : 0;
            rec->ref_end = hit ? (int)e.ref_pos + 1 : 0;
            if (Rp[half] == 0) {
                rec->gscore = 0;
                rec->gref_end = 0;
            }
        }
        const int last_row = Rp[half] - 1;
        if (last_row >= 0 && last_row / K == l) {
            int gs = 0, gt = 0;
#pragma unroll
            for (int q = 0; q < K; ++q) {
                if (q == last_row % K) {
                    gs = half ? rb[q].y : rb[q].x;
                    gt = half ? fc[q].y : fc[q].x;
                }
            }
            rec->gscore = gs;
            rec->gref_end = gt - l + 1;             // step -> column, half-open: the border column is 0
        }
    }
}

// The instances: the four gap forms on the six full geometries (24 instances).  A call whose plan is another geometry is
// re-planned onto the next full one, as suboptimal scores are.
template <int G, int K, bool FULL>
const void *extend_kernel(int gaps);

#ifdef VALIGN_KERNEL_PART_TU
template <int G, int K, bool FULL>
const void *extend_kernel(int gaps) {
    const void *ext[4] = {};
    if constexpr (FULL) {
        ext[kGapLinear] = (const void *)&score_extend_kernel<G, K, kGapLinear>;
        ext[kGapSym] = (const void *)&score_extend_kernel<G, K, kGapSym>;
        ext[kGapAffine] = (const void *)&score_extend_kernel<G, K, kGapAffine>;
        ext[kGapAffineSym] = (const void *)&score_extend_kernel<G, K, kGapAffineSym>;
    }
    return gaps >= 0 && gaps < 4 ? ext[gaps] : nullptr;
}
#endif

// ... and their ZDROP forms (keys extend_zdrop > 0 and extend_zdrop_rows = 1): 24 more, on the same six geometries
template <int G, int K, bool FULL>
const void *extend_zdrop_kernel(int gaps);

#ifdef VALIGN_KERNEL_PART_TU
template <int G, int K, bool FULL>
const void *extend_zdrop_kernel(int gaps) {
    const void *dropping[4] = {};
    if constexpr (FULL) {
        dropping[kGapLinear] = (const void *)&score_extend_kernel<G, K, kGapLinear, true>;
        dropping[kGapSym] = (const void *)&score_extend_kernel<G, K, kGapSym, true>;
        dropping[kGapAffine] = (const void *)&score_extend_kernel<G, K, kGapAffine, true>;
        dropping[kGapAffineSym] = (const void *)&score_extend_kernel<G, K, kGapAffineSym, true>;
    }
    return gaps >= 0 && gaps < 4 ? dropping[gaps] : nullptr;
}
#endif

}  // namespace valign
