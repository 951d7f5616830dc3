// extend_align_kernels.hip.h -- extension alignments (valign_hip_align_extend_*): the alignment of an extension, from the anchor
// before read[0] and ref[0] to the end cell the end-bonus rule picks (include/valign_hip.h has the definition;
// tests/extend_align_ref.py restates it in numpy).
//
// Two kernels:
//   align_extend_fill_kernel   score_extend_kernel's sweep (extend_kernels.hip.h: signed saturating packed int16 cells, gap-priced
//                              borders, the read top-aligned in the lane tile, rb / fc first arg-max per row under the packed Fp
//                              mask) that also derives every cell's back pointer by the equality tests of align_fill_kernel /
//                              align_fill_affine_kernel (trace_kernels.hip.h) and streams them to the HBM pointer scratch in the
//                              wave-contiguous block layout of those kernels: K words per lane and 8-step block (linear), K words
//                              of H codes followed by K words of gap codes (affine).  It writes the extension record when asked,
//                              and the EndCell the walk starts from.
//   extend_walk_kernel         one lane per pair, from that EndCell back to the anchor (-1, -1): stored codes inside, the border
//                              followed on the border (UP on column -1, LEFT on row -1, always at H).  It writes the two
//                              right-justified gapped rows and the four coordinates as traceback_kernel does, at a row pitch of
//                              R + F + 1 bytes: an extension can take R + F columns (every base against a gap), one more than
//                              traceback_kernel's rows hold.  cigar_encode_kernel reads them unchanged.
//
// Codes.  Linear: 0 DIAG, 1 UP, 2 LEFT, DIAG before UP before LEFT on ties.  Affine: the H word holds 0 DIAG, 1 the vertical
// state, 2 the horizontal state (DIAG before vertical before horizontal), the gap word bit 0 "the vertical state was extended",
// bit 1 "the horizontal state was extended" -- an open wins a tie.  The gap states of the two borders are the value -32768, which
// the saturating adds keep there: the first interior cell of a row or column always opens.
// The sweep runs whole 8-step blocks (the steps behind the last column are masked), so the last block is stored like every other.
#pragma once

#include "extend_kernels.hip.h"

namespace valign {

struct ExtendAlignArgs {
    const uint8_t *reads;     // n * R bytes, pair-major
    const uint8_t *refs;      // n * F bytes, pair-major
    unsigned *ptr;            // pointer scratch: [wave][block of steps][lane of the wave][words per block] dwords
    EndCell *ends;            // n: where each pair's walk starts ((-1, -1): the empty alignment)
    ExtendRec *extend;        // n, or null
    long long n;
    int R, F;
    int prof_area, refc_stride, wave_lds;
    int blocks8;              // 8-step blocks per lane = ceil((F + G - 1) / 8)
    int end_bonus;            // < 0: the best cell; >= 0: the read end where gscore + end_bonus >= score
    short match, mismatch;
    short gap_read, gap_ref;
    short open_read, ext_read, open_ref, ext_ref;
    int Z;                    // the ZDROP instances: extend_zdrop (> 0)
};

// a - b modulo 2^16 in each half: zero exactly where the two cells are equal, whatever their signs
__device__ __forceinline__ s16x2 pk_sub_wrap(s16x2 a, s16x2 b) { return (s16x2)((u16x2)a - (u16x2)b); }

// ZDROP (keys extend_zdrop > 0 and extend_zdrop_rows = 1): the same sweep and pointer stream; the epilogue takes the record from
// extend_zdrop_rows_record (extend_kernels.hip.h) -- the walk starts in the best cell before the drop row T, from where it only
// moves up and left, and the end-bonus rule picks the read end only where nothing dropped.
template <int G, int K, bool AFFINE, bool ZDROP = false>
__global__ void __launch_bounds__(256)
align_extend_fill_kernel(const ExtendAlignArgs args) {
    using geo = Geo<G, K>;
    constexpr int W = AFFINE ? 2 * K : K;           // words per lane and block
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
    // columns after the last ACGT base of every reference in the wave are not swept: no end cell lies there and no walk enters them
    const int F = w.cols_used;

    // ---- trimmed lengths of the group's two pairs, as score_extend_kernel takes them ----
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
    // (constants of the packed pointer / arg-max arithmetic in VGPRs the optimiser cannot see through: align_fill_kernel)
    s16x2 one = pk(1), two = pk(2), four = pk(4), fifteen = pk(15);
    asm volatile("" : "+v"(one), "+v"(two), "+v"(four), "+v"(fifteen));

    // X(i, -1): a gap of i + 1 read bases against nothing; X(-1, -1) = 0; pad rows as row R - 1
    auto border_col = [&](int row) __attribute__((always_inline)) -> short {
        const int i = row < R ? row : R - 1;
        if (i < 0) return 0;
        return (short)(AFFINE ? args.open_ref + i * args.ext_ref : (i + 1) * args.gap_ref);
    };

    s16x2 Hl[K], El[AFFINE ? K : 1];
    s16x2 code_h[K], code_g[AFFINE ? K : 1], acc_h[K], acc_g[AFFINE ? K : 1];
    s16x2 rb[K], fc[K];
#pragma unroll
    for (int q = 0; q < K; ++q) {
        Hl[q] = pk(border_col(l * K + q));
        if (AFFINE) El[q] = pk(kLoses);
        code_h[q] = acc_h[q] = pk(0);
        if (AFFINE) code_g[q] = acc_g[q] = pk(0);
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

    unsigned *ptr_lane = pointer_stream_lane<G, K, W>(args.ptr, w.pair0, args.blocks8, lane);

    // LDS fetches run one step ahead of the arithmetic, as in score_extend_kernel
    unsigned pa[K / 2], pb[K / 2];
    unsigned ca_next, cb_next;
    {
        const unsigned ca = *(lds_cu8 *)(code_addr), cb = *(lds_cu8 *)(code_addr + 1);
        lds_load_lane<K>(lane_base + ca * geo::kPairStride, pa);
        lds_load_lane<K>(lane_base + cb * geo::kPairStride, pb);
        ca_next = *(lds_cu8 *)(code_addr + 2);
        cb_next = *(lds_cu8 *)(code_addr + 3);
    }

    auto step = [&](auto masked_tag, int t) __attribute__((always_inline)) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        const s16x2 diag0 = up0;
        // every lane takes part in the DPP moves, before the select on the lane's column
        up0 = group_prev_or<G>(h_last, lead_h, lmask);
        lead_h = pk_add_sat(lead_h, lead_step);
        s16x2 fup0 = pk(0);
        if (AFFINE) fup0 = group_prev_or<G>(f_last, lead_f, lmask);
        s16x2 S[K];
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
            // what every row needs of the previous column only
            s16x2 d[K], m[K];
#pragma unroll
            for (int q = 0; q < K; ++q) {
                d[q] = pk_add_sat(q == 0 ? diag0 : Hl[q - 1], S[q]);
                s16x2 e;
                if (AFFINE) {
                    const s16x2 e_open = pk_add_sat(Hl[q], o_read);
                    e = pk_max(pk_add_sat(El[q], e_read), e_open);
                    El[q] = e;
                    code_g[q] = pk_min_u(pk_sub_wrap(e, e_open), one);            // 1: E extended, 0: opened from H
                } else {
                    e = pk_add_sat(Hl[q], g_read);
                }
                m[q] = pk_max(d[q], e);
            }
            // the chain down the column; the equal cells are compared, not their differences' sizes: a wrapped subtraction is
            // zero exactly where the two are equal
            s16x2 h = up0, f = fup0;
#pragma unroll
            for (int q = 0; q < K; ++q) {
                if (AFFINE) {
                    const s16x2 f_open = pk_add_sat(h, o_ref);
                    f = pk_max(pk_add_sat(f, e_ref), f_open);
                    code_g[q] = pk_mad_u(code_g[q], two, pk_min_u(pk_sub_wrap(f, f_open), one));      // bit 1 E extended, bit 0 F extended
                } else {
                    f = pk_add_sat(h, g_ref);
                }
                h = pk_max(m[q], f);
                Hl[q] = h;
                const s16x2 nd = pk_min_u(pk_sub_wrap(h, d[q]), one);
                const s16x2 nf = pk_min_u(pk_sub_wrap(h, f), one);
                code_h[q] = (s16x2)((u16x2)nd << (u16x2)nf);      // nd * (1 + nf): 0 DIAG, 1 from above (F), 2 from the left (E)
                track(q, h);
            }
            h_last = h;
            f_last = f;
        }
        // pointer accumulators shift every step in every lane, so that bit positions depend on t only; columns outside
        // [0, F) leave don't-care bits that are never read back
#pragma unroll
        for (int q = 0; q < K; ++q) {
            acc_h[q] = pk_mad_u(acc_h[q], four, code_h[q]);
            if (AFFINE) acc_g[q] = pk_mad_u(acc_g[q], four, code_g[q]);
        }
        if ((t & 7) == 7) {
            unsigned w8[W];
#pragma unroll
            for (int q = 0; q < K; ++q) w8[q] = as_u32(acc_h[q]);
            if (AFFINE) {
#pragma unroll
                for (int q = 0; q < K; ++q) w8[K + q] = as_u32(acc_g[q]);
            }
            store_block_words<W>(pointer_stream_block<W>(ptr_lane, t >> 3), w8);
        }
        ++j;
        code_addr += 2;
    };

    const int steps = ((F + G - 1 + 7) / 8) * 8;      // whole 8-step blocks: at most args.blocks8 of them (F <= args.F)
    const int fill_end = G - 1 < steps ? G - 1 : steps;
    const int steady_end = F > fill_end ? F : fill_end;
    int t = 0;
    for (; t < fill_end; ++t) step(std::true_type{}, t);
    for (; t + 1 < steady_end; t += 2) {       // two steps per trip: loop-carried registers swap roles
        step(std::false_type{}, t);
        step(std::false_type{}, t + 1);
    }
    for (; t < steady_end; ++t) step(std::false_type{}, t);
    for (; t < steps; ++t) step(std::true_type{}, t);

    if constexpr (ZDROP) {
        const int price_ref = extend_zdrop_price(AFFINE ? args.ext_ref : args.gap_ref), price_read = extend_zdrop_price(AFFINE ? args.ext_read : args.gap_read);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            int T;
            const ExtendRec rec = extend_zdrop_rows_record<G, K>(rb, fc, half, lane, l, Rp[half], args.Z, price_ref, price_read, T);
            const long long pair = w.pair0 + 2 * grp + half;
            if (l != 0 || pair >= args.n) continue;
            if (args.extend) args.extend[pair] = rec;
            const int last_row = Rp[half] - 1;
            EndCell start{-1, -1, 0, 0};                                 // the empty alignment: M == 0 ends in the anchor
            if (last_row >= 0 && !extend_zdrop_unreached(T, Rp[half]) && args.end_bonus >= 0 && (long long)rec.gscore + args.end_bonus >= (long long)rec.score)
                start = EndCell{(short)last_row, (short)(rec.gref_end - 1), (short)rec.gscore, 0};
            else if (rec.score > 0)
                start = EndCell{(short)(rec.read_end - 1), (short)(rec.ref_end - 1), (short)rec.score, 0};
            args.ends[pair] = start;
        }
        return;
    }
    // ---- the best cell > 0 of each pair (write_end_cells: into the wave's LDS table; no pad rows above the read) ----
    FillArgs fa{};
    fa.n = args.n;
    EndCell *wave_ends = reinterpret_cast<EndCell *>(w.first_bad);      // kPairs x 8 bytes behind the wave's tables, unused by this sweep
    const int none[2] = {0, 0};
    write_end_cells<G, K, kAlgSW>(fa, w, rb, fc, none, none, 0, lane, grp, l, 0, wave_ends);
    // ---- the records and the walk's start.  Row Rp - 1's entry (gscore and its column) comes to the group leader by a
    // shuffle every lane takes part in; the leader, which wrote the best cell into the wave's table, applies the end-bonus rule ----
    const int base_lane = lane - l;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const long long pair = w.pair0 + 2 * grp + half;
        const int last_row = Rp[half] - 1;
        const int own_row = last_row < 0 ? 0 : last_row;
        int gs = 0, gt = 0;
#pragma unroll
        for (int q = 0; q < K; ++q) {
            if (q == own_row % K) {
                gs = half ? rb[q].y : rb[q].x;
                gt = half ? fc[q].y : fc[q].x;
            }
        }
        const int gscore = __shfl(gs, base_lane + own_row / K, kWave);
        const int gref_end = __shfl(gt, base_lane + own_row / K, kWave) - own_row / K + 1;      // step -> column, half-open: the border column is 0
        if (l != 0 || pair >= args.n) continue;
        const EndCell e = wave_ends[2 * grp + half];                 // (this lane wrote the entry)
        const bool hit = e.score > 0 && last_row >= 0;
        const int score = hit ? (int)e.score : 0;
        if (args.extend) {
            ExtendRec rec;
            rec.score = score;
            rec.read_end = hit ? (int)e.read_pos + 1 : 0;
            rec.ref_end = hit ? (int)e.ref_pos + 1 : 0;
            rec.gscore = last_row >= 0 ? gscore : 0;
            rec.gref_end = last_row >= 0 ? gref_end : 0;
            args.extend[pair] = rec;
        }
        EndCell start{-1, -1, 0, 0};                                 // the empty alignment
        if (last_row >= 0 && args.end_bonus >= 0 && (long long)gscore + args.end_bonus >= (long long)score)
            start = EndCell{(short)last_row, (short)(gref_end - 1), (short)gscore, 0};
        else if (hit)
            start = EndCell{e.read_pos, e.ref_pos, e.score, 0};
        args.ends[pair] = start;
    }
}

struct ExtendWalkArgs {
    const uint8_t *reads;
    const uint8_t *refs;
    const unsigned *ptr;
    const EndCell *ends;
    uint8_t *rows;            // n * 2 * pitch; only the columns idx[0] .. idx[1] - 1 of a pair's two rows are written
    short *idx;               // n * 4: readStart, readEnd, refStart, refEnd (positions in the rows, traceback_kernel's format)
    long long n;
    int R, F;
    int G, K, blocks8;
    int affine;               // 1: pointer blocks hold K H-code words followed by K gap-code words
    int pitch;                // bytes of one row: R + F + 1
    int band_half;            // extend_band_walk_kernel (extend_band_align_kernels.hip.h): w of the band
};

// The register form's addressing for extend_walk_pair: [block of 8 steps][lane of the wave][wpb words] from the group's first lane
struct ExtendWalkLayout {
    int K, wpb, kGapWord;     // kGapWord: the gap codes' word lies this far behind the H codes' (affine)
    __device__ long long word(int i, int j, int &t) const {
        const int l = i / K, q = i - l * K;
        t = j + l;
        return ((long long)(t >> 3) * kWave + l) * wpb + q;
    }
};

// The walk of one pair, one lane.  A chain of dependent loads, as trace_walk is: pointer words are fetched 16 bytes at a time,
// bases 4 at a time, and the two output rows are written as dwords.  ptr_pair: the first word `layout` counts from, ptr_words:
// the words that may be read from there; layout.word(i, j, t): the word that holds the H code of the interior cell (i, j), and
// the step t whose bits are its.
template <class Layout>
__device__ __forceinline__ void extend_walk_pair(const ExtendWalkArgs &a, long long pair, const unsigned *ptr_pair, long long ptr_words, Layout &layout) {
    const int R = a.R, F = a.F;
    const int half_shift = (int)(pair & 1) * 16;
    const uint8_t *read = a.reads + pair * R, *ref = a.refs + pair * F;
    uint8_t *row_read = a.rows + pair * 2 * a.pitch, *row_ref = row_read + a.pitch;

    const EndCell e = a.ends[pair];
    int i = e.read_pos, j = e.ref_pos;
    int k = a.pitch - 2;
    long long cached_at = -1;              // first word index held in c0..c3 (multiple of 4)
    unsigned c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    int rd_at = -1, rf_at = -1;            // index / 4 of the cached read / ref dwords
    unsigned rd_w = 0, rf_w = 0;
    unsigned out_r = 0, out_f = 0;         // up to 4 pending output bytes per row, newest in the low byte
    int pending = 0;
    int state = 0;                         // affine only: 0 at H, 1 inside the vertical state, 2 inside the horizontal one

    auto base_at = [](const uint8_t *seq, int len, int pos, int &at, unsigned &w) -> unsigned {
        if ((pos >> 2) != at) {
            at = pos >> 2;
            const int b = at * 4;
            if (b + 4 <= len) {
                w = *reinterpret_cast<const u32_any_align *>(seq + b);
            } else {
                w = 0;
                for (int x = 0; b + x < len; ++x) w |= (unsigned)seq[b + x] << (8 * x);
            }
        }
        return (w >> (8 * (pos & 3))) & 0xFFu;
    };
    // 2-bit code of step t from word `wi` of this pair-of-pairs, through a 4-word cache
    auto code_at = [&](long long wi, int t) -> int {
        const long long wb = wi & ~3ll;
        if (wb != cached_at) {
            cached_at = wb;
            if (wb + 4 <= ptr_words) {
                const uint4 v = *reinterpret_cast<const uint4 *>(ptr_pair + wb);
                c0 = v.x; c1 = v.y; c2 = v.z; c3 = v.w;
            } else {
                c0 = ptr_pair[wb];
                c1 = wb + 1 < ptr_words ? ptr_pair[wb + 1] : 0u;
                c2 = wb + 2 < ptr_words ? ptr_pair[wb + 2] : 0u;
                c3 = 0u;
            }
        }
        const int sel = (int)(wi & 3);
        const unsigned word = sel == 0 ? c0 : (sel == 1 ? c1 : (sel == 2 ? c2 : c3));
        return (int)((word >> (half_shift + 2 * (7 - (t & 7)))) & 3u);
    };

    while ((i >= 0 || j >= 0) && k >= 0) {
        int move;                                       // 0 DIAG, 1 UP (a read base against '-'), 2 LEFT
        if (j < 0) {
            move = 1;                                   // the border column: UP to the anchor, at H
            state = 0;
        } else if (i < 0) {
            move = 2;                                   // the border row: LEFT to the anchor, at H
            state = 0;
        } else {
            int t;
            const long long wi = layout.word(i, j, t);
            if (!a.affine) {
                move = code_at(wi, t);
            } else if (state == 0) {
                move = code_at(wi, t);                  // 0 DIAG, 1 enter the vertical state, 2 enter the horizontal one
                if (move != 0) {
                    state = move;                       // nothing is emitted on entering a gap state
                    continue;
                }
            } else {
                const int bits = code_at(wi + layout.kGapWord, t);    // bit 0: vertical state extended, bit 1: horizontal state extended
                move = state;
                if (!(bits & state)) state = 0;         // opened here: back to H behind this column
            }
        }
        unsigned br, bf;
        if (move == 0) {
            br = base_at(read, R, i, rd_at, rd_w);
            bf = base_at(ref, F, j, rf_at, rf_w);
            --i;
            --j;
        } else if (move == 1) {
            br = base_at(read, R, i, rd_at, rd_w);
            bf = '-';
            --i;
        } else {
            br = '-';
            bf = base_at(ref, F, j, rf_at, rf_w);
            --j;
        }
        out_r = (out_r << 8) | br;
        out_f = (out_f << 8) | bf;
        if (++pending == 4) {                           // bytes k .. k+3 of both rows, lowest address = newest
            *reinterpret_cast<u32_any_align *>(row_read + k) = out_r;
            *reinterpret_cast<u32_any_align *>(row_ref + k) = out_f;
            pending = 0;
        }
        --k;
    }
    for (int x = 0; x < pending; ++x) {                 // k + 1 is the newest byte written
        row_read[k + 1 + x] = (uint8_t)(out_r >> (8 * x));
        row_ref[k + 1 + x] = (uint8_t)(out_f >> (8 * x));
    }
    short *out = a.idx + pair * 4;
    out[0] = (short)(k + 1);
    out[1] = (short)(a.pitch - 1);
    out[2] = (short)(k + 1);
    out[3] = (short)(a.pitch - 1);
}

#ifdef VALIGN_TU_EXTEND_ALIGN      // not a template: defined once, in engine_extend_align.hip
// One lane per pair.
__global__ void __launch_bounds__(256)
extend_walk_kernel(const ExtendWalkArgs a) {
    const long long pair = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= a.n) return;
    const int K = a.K, G = a.G;
    const int wpb = a.affine ? 2 * K : K;
    // pointer stream: [wave][block][lane of the wave][wpb]; this pair's group starts at lane (pair-of-pairs % groups) * G
    const int ppw = 2 * (kWave / G);
    const unsigned *ptr_pair = a.ptr + ((pair / ppw) * a.blocks8 * kWave + ((pair % ppw) >> 1) * G) * (long long)wpb;
    const long long ptr_words = ((long long)(a.blocks8 - 1) * kWave + G) * wpb;      // words from there to the end of the group's last block
    ExtendWalkLayout layout{K, wpb, K};
    extend_walk_pair(a, pair, ptr_pair, ptr_words, layout);
}
#endif

// The instances: linear and affine gaps on the six full geometries (12 instances).  A call whose plan is another geometry is
// re-planned onto the next full one, as extension scores are.
template <int G, int K, bool FULL>
const void *extend_align_kernel(int affine);

#ifdef VALIGN_KERNEL_PART_TU
template <int G, int K, bool FULL>
const void *extend_align_kernel(int affine) {
    const void *fill[2] = {};
    if constexpr (FULL) {
        fill[0] = (const void *)&align_extend_fill_kernel<G, K, false>;
        fill[1] = (const void *)&align_extend_fill_kernel<G, K, true>;
    }
    return affine == 0 || affine == 1 ? fill[affine] : nullptr;
}
#endif

// ... and their ZDROP forms: 12 more, on the same six geometries
template <int G, int K, bool FULL>
const void *extend_align_zdrop_kernel(int affine);

#ifdef VALIGN_KERNEL_PART_TU
template <int G, int K, bool FULL>
const void *extend_align_zdrop_kernel(int affine) {
    const void *dropping[2] = {};
    if constexpr (FULL) {
        dropping[0] = (const void *)&align_extend_fill_kernel<G, K, false, true>;
        dropping[1] = (const void *)&align_extend_fill_kernel<G, K, true, true>;
    }
    return affine == 0 || affine == 1 ? dropping[affine] : nullptr;
}
#endif

}  // namespace valign
