// long_plan.h -- the long-read path of a score call (Engine::score_long_device) before its launches: what the call is
// (LongScoreMode), which kernel instances are compiled for it, what the row strips keep in the boundary-row scratch, and the plan
// of the banded block chain (windows, period, delays, rings).  Integers in, integers out; no HIP (tests/long_plan_check.cpp
// exercises it on the CPU, tools/band_schedule_model.py states the chain's schedule in Python).
#pragma once

#include <stddef.h>

#include <algorithm>
#include <vector>

#include "band_window.h"
#include "cell_rules.h"

namespace valign {

constexpr int kPlanWave = 64;                       // lanes of a wave (kWave of the kernel headers)
constexpr int kLongG = 16, kLongK = 10;             // 160-row strips: the blocks the strip band is defined on, eight pairs per wave
constexpr int kLongTallG = 64, kLongTallK = 8;      // 512-row strips for unbanded sweeps of reads beyond two of them
constexpr int kPhase = 64;                          // steps between the ring refills of score_long_kernel; must be >= G - 1
constexpr int kBandG = 32;                          // block chain: lanes per group, two groups (= two pairs at a time) per wave
constexpr int kBandGroups = 2;
constexpr int kBandK = VALIGN_HIP_BAND_CHAIN_BLOCK_ROWS;       // rows per block = the band definition's block (describe: band_block_rows)
constexpr int kBandSlabs = 4 * kBandGroups + 1;     // (class, group) + one all-zero slab (both groups)
static_assert(kLongG * kLongK == VALIGN_HIP_BAND_BLOCK_ROWS, "banded strips are the API's blocks");
static_assert(kBandG * kBandGroups == kPlanWave, "the groups of the chain make a wave");

// ---- the route ----
enum class LongCells { F16, Int16, Int32 };
inline const char *long_cells_name(LongCells c) { return c == LongCells::F16 ? "f16" : (c == LongCells::Int16 ? "int16" : "int32"); }

// What the route reads of the engine beyond the rule inputs (Engine::long_facts)
struct LongFacts {
    int band_width = 0;
    bool band_nw = false;           // band_nw = 1: the band also applies to the NW variant
    bool wide = false;              // score_width asks for int32 cells, or the shape could leave int16 (Engine::score_wide_cells)
    bool short_strips = false, no_single_strip = false, no_band_chain = false;      // debug switches
    bool chain_usable = false;      // band_chain_plan(...).usable for this band_width
};

// What a long-read score call is.  long_score_mode() is the only place the route is decoded.
// chain: the banded block chain (G x K: its groups and blocks), else row strips of G x K rows; sym: one gap score (affine: one
// opening and one extension) both ways; single: the read is ONE 160-row strip; nw_band: the NW variant under the band;
// brow: the launches hand boundary rows on through the HBM scratch (the host pipeline keeps such calls on one stream)
struct LongScoreMode {
    int alg = kAlgSW;
    bool chain = false;
    int G = kLongG, K = kLongK;
    LongCells cells = LongCells::Int16;
    bool affine = false, sym = false, single = false, nw_band = false;
    bool brow = true;
};

// refuse = false (describe(), and the host pipeline before the call it sizes): the route a refused call would have taken
inline LongScoreMode long_score_mode(const RuleInputs &in, int alg, const LongFacts &f, bool refuse = true) {
    const Scoring &sc = in.sc;
    const bool banded = f.band_width > 0;
    if (refuse && banded && alg != kAlgSW && !f.band_nw) throw std::runtime_error("band_width applies to Smith-Waterman scores only");
    LongScoreMode m;
    m.alg = alg;
    m.affine = sc.affine;
    m.sym = (sc.affine ? (sc.open_read == sc.open_ref && sc.ext_read == sc.ext_ref) : sc.gap_read == sc.gap_ref) && !in.no_sym;
    m.nw_band = banded && alg == kAlgNW && f.band_nw;
    if (refuse && m.nw_band) {
        band_nw_check(in.R, in.F, f.band_width);
        if (int32_refused(in))
            throw std::runtime_error("shape x scoring can leave the int32 range of the DP cells (read_length " + std::to_string(in.R) +
                                     ", ref_length " + std::to_string(in.F) + ")");
    }
    // banded: the cyclic block chain (int32 cells whatever score_width says: same results in the int16 range) where its plan
    // fits; it keeps nothing in HBM between its steps
    m.chain = banded && (alg == kAlgSW || f.band_nw) && !f.no_band_chain && f.chain_usable;
    if (m.chain) return LongScoreMode{alg, true, kBandG, kBandK, LongCells::Int32, m.affine, m.sym, false, m.nw_band, false};
    const bool wide = f.wide || m.nw_band;      // (the banded NW strips: int32 cells, whose sentinel needs no range rule)
    // Unbanded sweeps of reads beyond a few strips take the tall strips; a band is defined on the 160-row blocks.
    const bool tall = !banded && in.R > 2 * kLongTallG * kLongTallK && !f.short_strips;
    m.G = tall ? kLongTallG : kLongG;
    m.K = tall ? kLongTallK : kLongK;
    // One 160-row strip, packed cells, no band (short reads sent here for their reference's length): the instances without
    // boundary rings, which keep nothing in HBM between launches
    m.single = in.R <= kLongG * kLongK && !wide && !banded && !f.no_single_strip;
    // Half-float cells: Smith-Waterman with one gap score on the 160-row strips while every cell stays below 1024 -- short reads
    // against a reference the resident kernels' LDS cannot hold (150 x 8 000: 8.2 -> ~11 TCUPS)
    const bool f16 = !tall && alg == kAlgSW && !sc.affine && m.sym && !wide && !banded && !in.no_f16 && half_float_unit_exact(sc, in.R, in.F);
    m.cells = f16 ? LongCells::F16 : (wide ? LongCells::Int32 : LongCells::Int16);
    m.brow = !m.single;
    return m;
}

// The kernel instances that are compiled (engine_long.hip instantiates exactly these).  Strips: [affine][alg][sym][int16 / int32]
// at 16 x 10 and at 64 x 8; at 16 x 10 also the half-float instance (SW, one gap score) and its single-strip form, the eight
// single-strip instances on int16 cells and the four banded NW ones on int32 cells.  The chain: [affine][sym][NW variant], each in
// the unit-delay and the delay-ring form (the plan says which runs).
constexpr bool long_instance_exists(int G, int K, const LongScoreMode &m) {
    if (m.alg != kAlgSW && m.alg != kAlgNW) return false;
    if (m.chain) return G == kBandG && K == kBandK && m.cells == LongCells::Int32 && !m.single && m.nw_band == (m.alg == kAlgNW);
    const bool strips160 = G == kLongG && K == kLongK;
    if (!strips160 && !(G == kLongTallG && K == kLongTallK)) return false;
    if (m.nw_band) return strips160 && m.alg == kAlgNW && m.cells == LongCells::Int32 && !m.single;
    if (m.cells == LongCells::F16) return strips160 && m.alg == kAlgSW && !m.affine && m.sym;
    if (m.single) return strips160 && m.cells == LongCells::Int16;
    return true;
}

// The instances by number: bit 0 the algorithm, then sym, affine, single, nw_band, two bits of cells (strips; the chain's
// lookup numbers its own)
constexpr int kLongInstances = 3 << 5;
constexpr int long_instance_index(const LongScoreMode &m) { return m.alg | m.sym << 1 | m.affine << 2 | m.single << 3 | m.nw_band << 4 | (int)m.cells << 5; }
constexpr LongScoreMode long_instance_mode(int G, int K, int i) {
    return LongScoreMode{i & 1, false, G, K, (LongCells)(i >> 5), (i & 4) != 0, (i & 2) != 0, (i & 8) != 0, (i & 16) != 0, (i & 8) == 0};
}

// ---- the row strips' sizes ----
struct LongSizes {
    int rows = 0, strips = 0;       // rows per strip: G K; strips of the read
    int ppw = 0;                    // pairs per wave
    int row_dwords = 0;             // dwords per boundary row: F rounded up to kPhase, plus kPhase
    int row_sets = 0;               // boundary rows per pair-of-pairs: per half (int32 cells), H and F (affine)
    size_t bytes_per_wave = 0;      // the boundary rows of a wave's pairs, both buffers
    long long chunk = 0, waves = 0; // pairs per launch -- at most 8 GiB of boundary rows, whole waves -- and its waves
    long long pp_total = 0;         // pair-of-pairs slots of the scratch (LongArgs)
    size_t brow_bytes = 0;          // the scratch; 0: a single strip keeps none
};

inline LongSizes long_strip_sizes(int R, int F, long long n, const LongScoreMode &m) {
    LongSizes s;
    s.rows = m.G * m.K;
    s.strips = std::max(1, (R + s.rows - 1) / s.rows);
    s.ppw = 2 * (kPlanWave / m.G);
    s.row_dwords = ((F + m.G + kPhase - 1) / kPhase) * kPhase + kPhase;
    s.row_sets = (m.cells == LongCells::Int32 ? 2 : 1) * (m.affine ? 2 : 1);
    s.bytes_per_wave = (size_t)2 * (s.ppw / 2) * s.row_dwords * 4 * s.row_sets;
    s.chunk = (long long)((8ull << 30) / s.bytes_per_wave) * s.ppw;
    s.chunk = std::max<long long>(s.ppw, std::min(s.chunk, (n + s.ppw - 1) / s.ppw * s.ppw));
    s.waves = s.chunk / s.ppw;
    s.pp_total = s.waves * (s.ppw / 2) * s.row_sets;
    s.brow_bytes = m.brow ? (size_t)s.waves * s.bytes_per_wave : 0;
    return s;
}

// ---- the banded block chain (band_kernels.hip.h) ----
struct BandBlock {          // per row block, computed once on the host (band_chain_plan)
    int start;              // column of the block's first step (its window's first column - 1: the warm-up column)
    int lo;                 // first column of the window, clipped to the matrix (0x3FFFFFFF: nothing to compute)
    int span;               // last column - first column
    int delay;              // steps between the predecessor's write and this block's read of the same column
};

// LDS of one wave of score_band_kernel: the query profile, the reference rings, the delay rings
template <int K>
struct BandLds {
    static constexpr int kRowChunks = K / 8;
    static constexpr int kChunkBytes = kBandSlabs * kBandG * 16;          // one 8-row chunk (int16 scores) of every slab
    static constexpr int kProf = 0;
    static constexpr int kProfBytes = kRowChunks * kChunkBytes;
    // (the reference rings are addressed as base | column: aligned to their own size, code_cols a power of two)
    __host__ __device__ static int codes(int code_cols) { return (kProfBytes + code_cols - 1) / code_cols * code_cols; }
    // (the delay rings are addressed as base | offset: aligned to one lane's ring)
    __host__ __device__ static int ring(int code_cols, int ring_depth) {
        const int at = codes(code_cols) + kBandGroups * code_cols, a = ring_depth * 4;
        return (at + a - 1) / a * a;
    }
    // (ring_depth 0: the unit-delay kernel, no ring; affine: a second ring, for F, behind the first)
    __host__ __device__ static int total(int code_cols, int ring_depth, bool affine = false) {
        return ring(code_cols, ring_depth ? ring_depth : 1) + kPlanWave * ring_depth * 4 * (affine ? 2 : 1);
    }
};

struct BandPlan {
    bool usable = false, unit_delay = false;
    int nb = 0, first_block = 0, pad_rows = 0, d = 0, ring_depth = 0, code_cols = 0, events = 0;
    long long cells = 0;                // DP cells one pair's band windows hold (what the chain actually sweeps)
    std::vector<BandBlock> blocks;
    std::vector<int> fill_to;
};

// Windows, start distance, delays and ring sizes of the block chain for (R, F, band): what tools/band_schedule_model.py
// calls plan().  `usable` is false where the chain does not pay or does not fit (then score_long_kernel's strips run).
inline BandPlan band_chain_plan(int R, int F, int band_width, bool affine) {
    BandPlan p;
    const int w = band_width / 2, G = kBandG, K = kBandK;
    if (band_width <= 0 || R <= 0 || F <= 0) return p;
    const int rows = G * K;
    const int strips = std::max(1, (R + rows - 1) / rows);
    p.pad_rows = strips * rows - R;
    p.nb = strips * G;
    p.events = p.nb + G;
    std::vector<int> start((size_t)p.nb), lo((size_t)p.nb), hi((size_t)p.nb);
    int first_real = -1;
    for (int b = 0; b < p.nb; ++b) {
        int r_lo = b * K - p.pad_rows, r_hi = (b + 1) * K - p.pad_rows - 1;
        if (r_hi < 0) {                            // a block of padding rows only
            lo[(size_t)b] = 1;
            hi[(size_t)b] = 0;
            continue;
        }
        if (first_real < 0) first_real = b;
        r_lo = std::max(r_lo, 0);
        r_hi = std::min(r_hi, R - 1);
        const long long a = (long long)r_lo * F / R - w;
        start[(size_t)b] = (int)a - 1;             // the warm-up column: the diagonal neighbour of the window's first cell
        lo[(size_t)b] = (int)std::max<long long>(a, 0);
        hi[(size_t)b] = (int)std::min<long long>((long long)r_hi * F / R + w, F - 1);
    }
    for (int b = 0; b < first_real; ++b) start[(size_t)b] = start[(size_t)first_real];
    p.first_block = std::max(first_real, 0);
    int width = 1, dmax = 0, dmin = 1 << 30;
    for (int b = 0; b < p.nb; ++b) {
        width = std::max(width, hi[(size_t)b] - start[(size_t)b] + 1);
        if (b > first_real) {
            dmax = std::max(dmax, start[(size_t)b] - start[(size_t)b - 1]);
            dmin = std::min(dmin, start[(size_t)b] - start[(size_t)b - 1]);
        }
    }
    if (dmin > dmax) dmin = dmax;
    // A block reads its predecessor up to dmax steps late; by then the predecessor may have begun its next block, but only
    // with that block's warm-up step, which writes the 0 the band gives that cell: width + dmax - 1 steps per period
    // suffice -- and a lane finishes its own block first (tools/band_schedule_model.py).
    p.d = std::max((std::max(width, width + dmax - 1) + G - 1) / G, dmax + 1);
    // every block one step behind its predecessor on the same column: the cell travels by DPP, no ring (UNIT kernel);
    // otherwise the ring is read one step ahead, which needs every delay >= 2
    p.unit_delay = dmin == dmax && p.d == dmax + 1;
    if (!p.unit_delay) p.d = std::max(p.d, dmax + 2);
    const int delay_max = p.d - dmin;
    p.ring_depth = 4;
    while (p.ring_depth < delay_max + 1) p.ring_depth *= 2;
    p.blocks.assign((size_t)p.events + 2, BandBlock{0, 0x3FFFFFFF, 0, 1});
    for (int b = 0; b < p.nb; ++b) {
        BandBlock &k = p.blocks[(size_t)b];
        k.start = start[(size_t)b];
        if (lo[(size_t)b] <= hi[(size_t)b]) {
            k.lo = lo[(size_t)b];
            k.span = hi[(size_t)b] - lo[(size_t)b];
            const int r_lo = std::max(b * K - p.pad_rows, 0), r_hi = std::min((b + 1) * K - p.pad_rows - 1, R - 1);
            p.cells += (long long)(k.span + 1) * (r_hi - r_lo + 1);
        }
        // (blocks of padding write zeros whatever they are asked: their successor may read any slot)
        k.delay = b > first_real ? p.d - (start[(size_t)b] - start[(size_t)b - 1]) : 2;
    }
    // reference ring: by event e every column below fill_to[e] is in the ring -- what any running block reaches in the d
    // steps after the event plus the sweep's look-ahead of two; the ring must span from the newest block's column to there
    p.fill_to.assign((size_t)p.events + 2, 0);
    int reach = 0, span = 0;
    for (int e = 0; e <= p.events + 1; ++e) {
        int head = -(1 << 30), tail = 1 << 30;
        for (int b = std::max(0, e - G + 1); b <= std::min(e, p.nb - 1); ++b) {
            head = std::max(head, start[(size_t)b] + (e - b) * p.d);
            tail = std::min(tail, start[(size_t)b] + (e - b) * p.d);
        }
        if (head > -(1 << 30)) reach = std::max(reach, std::min(head + p.d + 3, F));
        p.fill_to[(size_t)e] = reach;
        if (tail < (1 << 30)) span = std::max(span, reach + 2 * G - std::max(tail, 0));     // (+ what one event may commit early)
        if (e > 0 && p.fill_to[(size_t)e] - p.fill_to[(size_t)e - 1] > 2 * G) return p;      // more than two rounds per event: not built
    }
    p.code_cols = 128;
    while (p.code_cols < span + 8) p.code_cols *= 2;
    // What the chain buys is the lane-steps outside the band; it pays while windows are narrow against a strip's slope.
    // Limits of the kernel: ring addressing (base | offset) and one CU's LDS.
    if (p.code_cols > 2048 || p.ring_depth > 64) return p;
    if (p.unit_delay) p.ring_depth = 0;
    if (BandLds<kBandK>::total(p.code_cols, p.ring_depth, affine) > 40 * 1024) return p;
    p.usable = true;
    return p;
}

}  // namespace valign
