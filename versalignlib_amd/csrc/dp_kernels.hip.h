// dp_kernels.hip.h -- gfx950 score kernels for the versalignLib AlignmentKernel path.
//
// What is computed (reference semantics, restated in oracle/cpu_ref.c):
//   Smith-Waterman score ........ src/Kernels/default/DefaultKernel.cpp:83-138
//   Needleman-Wunsch-variant .... src/Kernels/default/DefaultKernel.cpp:140-202
//   substitution classes ........ src/Kernels/default/DefaultKernel.h:43-60, 83-97
// plus an affine-gap (Gotoh) extension that the reference does not have.
//
// How (nothing here follows the reference's row-major sweeps or its OpenCL kernel):
//   * A lane GROUP of G lanes (G = 8/16/32/64, a slice of one wave64) owns TWO pairs
//     at once: every DP value is a packed 2 x int16 register, pair A in the low half,
//     pair B in the high half, so one v_pk_* instruction updates two cells.
//   * Lane l of the group owns K consecutive DP rows (register tile); the group sweeps
//     the reference left to right in a skewed (anti-diagonal) front: at step t lane l
//     works on reference column t - l.  The "left" dependency is a register, "up" is
//     the previous register of the same lane, and only the last row of each lane
//     travels to lane l+1 -- one DPP move per step, no LDS traffic for DP state.
//   * Rows are padded at the TOP (rows before the read starts carry class "none",
//     substitution 0): with non-positive gap scores those rows stay exactly at the
//     row-0 boundary value, so the real last row is always the last register of the
//     last lane and no per-cell row masking is needed.
//   * Substitution scores come from a per-pair query profile in LDS: four slabs
//     (A, T, C, G) of padded-rows x int16 per pair plus one all-zero slab shared by every
//     pair; the reference bases are staged once as slab numbers, so a lane's fetch address
//     is lane_base + slab * stride and its K scores arrive with the widest ds_read the
//     lane stride allows.  The slab stride carries the padding that a compile-time bank
//     model (profile_conflicts) finds conflict-free.  Inputs are raw ASCII as delivered
//     by the ABI (1 byte per base): refs via 16-byte coalesced loads, reads as coalesced
//     byte loads.
//     (The tilted int16 symmetric affine Smith-Waterman sweep keeps them in REGISTERS instead where every score is a
//     byte: four bytes per row and pair, looked up by the one v_perm_b32 the merge takes anyway, from a stream of
//     selector dwords -- wave_setup_tables; no profile, no slab numbers.  One tile exists for that form alone: 8 lanes x 19 rows,
//     152 rows for reads of 129 .. 152 bases, 16 pairs per wave, its stream 16 bits per column -- cell_constants.h: tilt_tables_only.
//     Its lane groups INTERLEAVE, two to a 16-lane DPP row on alternating lanes, so that the row's boundary is the groups' and
//     each lane hand-over of a step is one DPP instruction -- lane_map.h; every other kernel keeps contiguous groups.)
//   * Recurrence variants (GAPS), packed instructions per register (= per two cells) incl. the
//     profile merge: two linear gap scores 6 + maximum tracking, one shared gap score 5 +
//     tracking, affine 10 + tracking, affine with the same open/extend for both directions 9 + tracking (Smith-Waterman:
//     inside the window of its biased form 8 + 1/2 -- every int16 cell kept as value + B, maxima three at a time through
//     v_pk_maximum3_f16, which is an integer maximum on bit patterns in [0x0400, 0x7BFF]; with at most 12 rows per lane
//     and a little further inside that window 6 + (K / 2 + 4) / K: the same biased cells in a TILTED frame, value + B +
//     x (p + j + c0), where an extension costs nothing and the zero floor is a register that moves with the frame; beyond
//     the window 9 on gap SOURCES, tracked once per two steps -- 9 + (K + 1) / 2K; see score_kernel's sweep).  Where every
//     cell provably stays a small integer the same recurrences run on packed HALF FLOATS, which
//     gfx950 gives a three-operand maximum (v_pk_maximum3_f16) and a free [0, 1] clamp on the
//     add: shared-gap linear SW 4 (keeps (h, max(h + g, 0)) scaled by 2^-10), symmetric affine 8,
//     affine 9 -- results identical to the int16 forms, which remain the fallback.  The SW maximum
//     is tracked on diag+S, off the dependency chain.
//   * The NW variant (no zero floor) runs every recurrence in a TILTED FRAME, cell (p, j) kept as
//     V - g_ref * p - g_read * j: gap steps (affine: extensions) cost nothing, the diagonal pays for
//     both through the query profile -- linear 3 packed instructions per register on half floats
//     (perm, add, max3), 4 on int16; symmetric affine 6 / 7.  See score_kernel.
//   * Smith-Waterman sweeps run unmasked from the first step to the last: a lane outside columns [0, F) reads
//     zero-slab codes from the pads of the code array, stays zero before column 0 and can only repeat values that
//     exist already after column F-1, so no step needs a mask and the whole sweep is one loop of two-step trips,
//     started at the first lane that owns a real row.  The NW variant keeps EXEC-masked fill / drain steps: its
//     result reads every lane's registers frozen at the last column.  The set-up before a sweep (wave_setup) works
//     a dword at a time: four reference columns, four read rows per lane and trip (base_classes.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "base_classes.h"
#include "cell_constants.h"
#include "lane_map.h"

namespace valign {

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

constexpr int kWave = 64;
constexpr int kWaveLanes = 64;
constexpr int kCodePad = 72;          // columns of zero-slab codes before column 0 and after column F-1
constexpr short kNegInf = -16384;   // "minus infinity" of the affine NW borders (oracle: NEG_INF)

constexpr int kMaxScoreGroups = 16;
constexpr int kOneSweep = 0x7FFFFFFF;      // wave_setup: the sweep covers the whole read (padding rows on top)

struct ScoreArgs {
    const uint8_t *reads;     // n * R bytes, pair-major
    const uint8_t *refs;      // n * F bytes, pair-major
    int16_t *scores;          // n
    long long n;
    int R, F;
    int prof_area;            // bytes reserved for the profile (>= raw-ref staging it aliases)
    int refc_stride;          // bytes of one group's interleaved class-code array
    int wave_lds;             // bytes of LDS per wave
    short match, mismatch;
    union {
        struct {
            short gap_read, gap_ref;               // linear model, all <= 0
        };
        // The affine kernels never read the linear model.  A launch of score_kernel<G, K, kAlgSW, kGapAffineSym> carries in
        // its place what selects the form of that sweep: > 0 the biased three-operand-maximum form, and its bias B (cell_rules.h:
        // sym_affine_max3_ok / sym_affine_bias); 0 the gap-source form.  No offset and no size changes for any kernel.
        // Bit 16 set: the biased form in its tilted frame, the low 16 bits its bias (sym_affine_tilt_ok / sym_affine_tilt_bias).
        int sym_max3_bias;
    };
    short open_read, ext_read, open_ref, ext_ref;  // affine extension, all <= 0
    // Length-sorted batches (ragged_kernels.hip.h; Engine::ragged_finish): one launch sweeps several packed groups
    // of pairs that share the read stride R but have their own reference stride.  Blocks
    // [groups[g-1].block_end, groups[g].block_end) belong to group g; reads / refs / scores / n / F
    // above are then ignored in favour of the group's.  n_groups == 0: one plain batch.
    int n_groups;
    struct Group {
        unsigned block_end;
        int F;
        long long n;
        long long pair_ofs;         // into scores
        long long read_ofs, ref_ofs;   // bytes into reads / refs
    } groups[kMaxScoreGroups];
    // Behind everything else, so that no other member moves: two device words the 8 x 19 instance (the only one that reads this
    // member) reports its form in -- a wave that ran the plain row-table step sets word 0, one that ran the repairing copy word 1
    // (describe: ran_score_sym_affine_form).  Null: nothing is reported.
    unsigned *form_seen;
};

// ---- packed int16 helpers (each is one VOP3P instruction on gfx950) ----
__device__ __forceinline__ s16x2 pk(short v) { return s16x2{v, v}; }
__device__ __forceinline__ s16x2 pk_max(s16x2 a, s16x2 b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ s16x2 pk_add_sat(s16x2 a, s16x2 b) { return __builtin_elementwise_add_sat(a, b); }
// max(a - g, 0) on non-negative a with magnitude g: v_pk_sub_u16 ... clamp
__device__ __forceinline__ s16x2 pk_sub_floor0(s16x2 a, s16x2 g) {
    return (s16x2)__builtin_elementwise_sub_sat((u16x2)a, (u16x2)g);
}
__device__ __forceinline__ unsigned as_u32(s16x2 v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ s16x2 as_pk(unsigned v) { return __builtin_bit_cast(s16x2, v); }

// value of lane-1 (wave-wide shift right by one lane); lane 0 receives 0
__device__ __forceinline__ unsigned from_prev_lane(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}

// value of the previous lane of the lane's G-lane group, 0 in the group's first lane.  Groups of 16 are the DPP rows:
// row_shr:1 with bound_ctrl is exactly that in ONE instruction (else: wave-wide shift, then the mask)
template <int G>
__device__ __forceinline__ unsigned group_prev_or_zero(unsigned v, unsigned lmask) {
    if (G == 16) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /* row_shr:1 */, 0xF, 0xF, true);
    return from_prev_lane(v) & lmask;
}

// ... and a border value instead of 0 in the group's first lane; `lead_border` holds it in that lane and 0 in every other.
// Groups of 16: OR-ed onto the zero that row_shr:1 with bound_ctrl delivers there, which folds into ONE v_or_b32 with a DPP
// operand (a DPP move that keeps `old` would need a copy of the border in front of it)
// (every lane takes part in the shift: the move is never written under a lane condition)
template <int G>
__device__ __forceinline__ s16x2 group_prev_or(s16x2 v, s16x2 lead_border, unsigned lmask) {
    return as_pk(group_prev_or_zero<G>(as_u32(v), lmask) | as_u32(lead_border));
}
// The same two hand-overs under the INTERLEAVED lane map (lane_map.h: the S = 16 / G groups of a DPP row on alternating lanes).
// The previous lane of the group is lane - S in the same row and the leaders are the row's first S lanes, which row_shr:S with
// bound_ctrl zeroes: ONE v_mov_b32_dpp whatever the group size, no mask; the border form folds into ONE v_or_b32 with a DPP
// operand as it does for contiguous groups of 16.
template <int S>
__device__ __forceinline__ unsigned row_prev_or_zero(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + S /* row_shr:S */, 0xF, 0xF, true);
}
template <int S>
__device__ __forceinline__ s16x2 row_prev_or(s16x2 v, s16x2 lead_border) {
    return as_pk(row_prev_or_zero<S>(as_u32(v)) | as_u32(lead_border));
}
// max(a, b) and max(a, b, c) of int16 values whose bit patterns all lie in [0x0400, 0x7BFF], the positive normal half floats:
// there the half-float order is the integer order and a maximum returns one of its operands bit for bit, so gfx950's
// v_pk_maximum3_f16 is an integer maximum of three
__device__ __forceinline__ s16x2 pk_max_h(s16x2 a, s16x2 b) {
    return __builtin_bit_cast(s16x2, __builtin_elementwise_maximum(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b)));
}
__device__ __forceinline__ s16x2 pk_max3_h(s16x2 a, s16x2 b, s16x2 c) {
    return __builtin_bit_cast(s16x2, __builtin_elementwise_maximum(__builtin_elementwise_maximum(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b)),
                                                                  __builtin_bit_cast(f16x2, c)));
}

// fn(integral_constant<int, 0>), fn(integral_constant<int, 1>), ...: a loop whose counter is a compile-time constant in every pass
template <int... Is, class Fn>
__device__ __forceinline__ void unrolled_steps(std::integer_sequence<int, Is...>, Fn &&fn) {
    (fn(std::integral_constant<int, Is>{}), ...);
}

// LDS bank conflicts of one profile fetch, modelled per MI355X_MICROARCH.md section LDS: every lane of
// a group of G reads `lane_dw` dwords at dword address slab(pair of its group) * stride + l * lane_dw.
// width = dwords per load instruction (1: ds_read_b32 / read2_b32, banks mod 32, lane groups of 32;
// 2: ds_read_b64, banks mod 64, groups of 32; 4: ds_read_b128, banks mod 64, four fixed groups of 16).
// Returns the number of extra LDS cycles when every lane selects the same class (the systematic case).
constexpr int profile_conflicts(int G, int lane_dw, int width, int stride_dw) {
    const int banks = width == 1 ? 32 : 64;
    int extra = 0;
    const int ngroups = width == 4 ? 4 : 2;
    for (int grp = 0; grp < ngroups; ++grp) {
        int hits[64] = {};
        int worst = 0;
        for (int lane = 0; lane < kWaveLanes; ++lane) {
            int member = 0;
            if (width == 4) {
                const int m = lane & 31;                       // {0-3,12-15,20-27} vs the rest, per half
                const bool first = m < 4 || (m >= 12 && m < 16) || (m >= 20 && m < 28);
                member = (lane < 32 ? 0 : 2) + (first ? 0 : 1);
            } else {
                member = lane / 32;
            }
            if (member != grp) continue;
            const int l = lane % G, pair = 2 * (lane / G);
            const int dw = pair * stride_dw + l * lane_dw;
            for (int x = 0; x < width; ++x) {
                const int b = (dw + x) % banks;
                hits[b] += 1;
                worst = hits[b] > worst ? hits[b] : worst;
            }
        }
        extra += worst - 1;
    }
    return extra;
}

// Geometry of one kernel instantiation.
template <int G, int K>
struct Geo {
    static_assert(G == 4 || G == 8 || G == 16 || G == 32 || G == 64, "group size");
    // (8 x 19, the row-table tile of the tilted symmetric affine sweep, builds no profile: kNoProfile leaves the slab constants out)
    static constexpr bool kNoProfile = tilt_tables_only(G, K);
    static_assert(K % 2 == 0 || kNoProfile, "rows per lane must be even");
    static constexpr int kGroups = kWave / G;        // lane groups per wave
    static constexpr int kPairs = 2 * kGroups;       // pairs per wave
    static constexpr int kRows = G * K;              // padded rows
    static constexpr int kLaneBytes = K * 2;         // one lane's K int16 scores, contiguous
    static constexpr int kLoadDwords = (K * 2) % 16 == 0 ? 4 : ((K * 2) % 8 == 0 ? 2 : 1);
    // Slab stride: the rows plus the padding (in units of one load) that minimises the systematic
    // bank conflicts between the lane groups of a wave (e.g. 16x10: 80 -> 88 dwords turns an
    // always-2-way conflict between groups 0/1 and 2/3 into none).
    static constexpr int slab_dwords() {
        const int rows_dw = kRows / 2;
        int best = rows_dw, best_cost = profile_conflicts(G, K / 2, kLoadDwords, rows_dw);
        for (int pad = kLoadDwords; pad < 64 && best_cost > 0; pad += kLoadDwords) {
            const int c = profile_conflicts(G, K / 2, kLoadDwords, rows_dw + pad);
            if (c < best_cost) {
                best_cost = c;
                best = rows_dw + pad;
            }
        }
        return best;
    }
    static constexpr int kPairStride = kNoProfile ? 0 : slab_dwords() * 4;   // bytes of one (class, pair) slab
    // profile slabs: slab (class * kPairs + pair) for classes 0..3, plus ONE all-zero slab
    // shared by every pair for "this reference base scores nothing"
    static constexpr int kZeroSlab = 4 * kPairs;
    static constexpr int kProfBytes = (4 * kPairs + 1) * kPairStride;
    // byte offset of row q of lane l inside one (class, pair) array
    __host__ __device__ static constexpr int row_offset(int l, int q) { return l * kLaneBytes + q * 2; }
};

typedef __attribute__((address_space(3))) const unsigned lds_cu32;
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const u32x2 lds_cu32x2;
typedef __attribute__((address_space(3))) const u32x4 lds_cu32x4;
typedef __attribute__((address_space(3))) const unsigned char lds_cu8;

// LDS byte offset of a pointer into the dynamic shared array
__device__ __forceinline__ unsigned lds_offset(const void *p) {
    return (unsigned)(size_t)(__attribute__((address_space(3))) const void *)p;
}

// Copy global bytes [begin, end) of `src` into LDS so that byte x lands at
// dst[x - (begin & ~15)] : 16-byte coalesced loads for the interior, bytes at the rims.
__device__ __forceinline__ void stage_span(unsigned char *dst, const uint8_t *src, long long begin,
                                           long long end, int lane) {
    const unsigned long long a0 = (unsigned long long)(src + begin) & ~15ull;
    const unsigned long long lo = (unsigned long long)(src + begin);
    const unsigned long long hi = (unsigned long long)(src + end);
    for (unsigned long long a = a0 + 16ull * lane; a < hi; a += 16ull * kWave) {
        unsigned char *d = dst + (a - a0);
        if (a >= lo && a + 16 <= hi) {
            *reinterpret_cast<uint4 *>(d) = *reinterpret_cast<const uint4 *>(a);
        } else {
            for (int b = 0; b < 16; ++b)
                if (a + b >= lo && a + b < hi) d[b] = *reinterpret_cast<const uint8_t *>(a + b);
        }
    }
}

// The four LDS bytes that start at `p`, whatever its alignment: the two aligned dwords around them, one v_alignbyte_b32
// (reads up to 7 bytes past p: callers keep that inside the wave's LDS)
__device__ __forceinline__ unsigned lds_dword_at(const unsigned char *p) {
    const unsigned a = lds_offset(p), base = a & ~3u;
    const unsigned lo = *(lds_cu32 *)(base), hi = *(lds_cu32 *)(base + 4);
    return __builtin_amdgcn_alignbyte(hi, lo, a & 3u);
}

extern __shared__ __align__(16) unsigned char valign_smem[];

// Per-wave LDS tables shared by the score and the alignment-fill kernels.
struct WaveTables {
    unsigned char *prof;    // [4 classes x pairs + 1 zero slab][lane rows] int16 substitution scores
    unsigned char *refc;    // [groups][2 * F] profile slab numbers, pair A / pair B interleaved
    int *first_bad;         // [pairs][2]: first read / ref position whose class is 0 (else R / F)
    long long pair0;        // first pair of this wave
    int last;               // index of the last existing pair of the wave (tail waves are short)
    int cols_used;          // 1 + last column where any pair of the wave has an ACGT base (wave-uniform)
};

// Stage the wave's raw refs with coalesced 16-byte loads, then build the per-column slab
// numbers and the query profile.  Both go a dword at a time (base_classes.h: base_class4): a lane turns four
// reference columns of pair A and of pair B into four interleaved slab-number pairs (the rim F % 4 goes byte-wise),
// and four rows of a read into the 4 x 4 scores of the four class slabs, looked up with v_perm_b32 from eight-entry
// tables indexed by the class.  The wave's reads are one contiguous span when one sweep covers the read: it is staged
// beside the references where both fit the profile area; otherwise (row strips, long references) the read bases
// come straight from HBM, one coalesced byte per lane and row.  Returns false for a wave past the end of the
// batch (it still takes part in the block barriers).
template <int G, int K, bool FIND_BAD>
__device__ __forceinline__ bool wave_setup(const uint8_t *reads, const uint8_t *refs, long long n, int R, int F,
                                           int prof_area, int refc_stride, int wave_lds, short match,
                                           short mismatch, WaveTables &w, bool bad_is_non_acgt = false,
                                           unsigned block = blockIdx.x, short zero_score = 0,
                                           int strip_row0 = kOneSweep, short row_key_step = 0, short row0_score = 0) {
    using geo = Geo<G, K>;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    // read position of padded row 0 of this sweep: -(padding rows) when one sweep covers the read; a row strip
    // of a longer read (strip_kernels.hip.h) starts wherever it starts, rows outside [0, R) are padding
    const int row0 = strip_row0 == kOneSweep ? R - geo::kRows : strip_row0;

    unsigned char *lds = valign_smem + (size_t)wave * wave_lds;
    unsigned char *prof = lds;
    unsigned char *refc = lds + prof_area;
    int *first_bad = reinterpret_cast<int *>(refc + geo::kGroups * refc_stride);

    const int waves = blockDim.x / kWave;
    const long long pair0 = ((long long)block * waves + wave) * geo::kPairs;
    const bool live = pair0 < n;
    long long pair_end = pair0 + geo::kPairs;
    if (pair_end > n) pair_end = n;
    const int last = (int)(pair_end - pair0) - 1;

    // (where all the wave's references fit the profile area anyway -- 8 x 500 bytes in 11.6 KB -- they are staged in one go:
    // one barrier instead of two per lane group, 1.5 % of the 150 x 500 sweep)
    const bool whole = geo::kPairs * F + 32 <= prof_area;
    // ... and the wave's reads behind them (8 x 150 bytes), when one sweep covers the read
    const int rd_off = ((geo::kPairs * F + 32 + 15) / 16) * 16;
    const bool rd_staged = whole && strip_row0 == kOneSweep && rd_off + geo::kPairs * R + 32 <= prof_area;

    // ---- otherwise: read bases of this lane's 2K (pair, padded row) items, straight from HBM ----
    // kPairs * kRows == 128 * K for every geometry, so each lane owns exactly 2K items.
    unsigned char rd[2 * K];
    if (live && FIND_BAD && lane < geo::kPairs) {
        first_bad[2 * lane] = R;
        first_bad[2 * lane + 1] = F;
    }
    if (live && !rd_staged) {
#pragma unroll
        for (int i = 0; i < 2 * K; ++i) {
            const int idx = lane + kWave * i;
            const int p = idx / geo::kRows, rr = idx - p * geo::kRows;
            const int ps = p > last ? last : p;
            const int pos = row0 + rr;
            rd[i] = (pos >= 0 && pos < R) ? reads[(pair0 + ps) * R + pos] : (unsigned char)0;
        }
    }

    // ---- reference bases -> profile slab of the pair (class * kPairs + pair, or the zero slab) ----
    // One lane group after the other: the group's two raw references are staged in the (not yet built) profile area -- 2 F
    // bytes instead of the wave's 2 F x groups (round 4: that staging, not the tables, was what a long reference cost first:
    // 150 x 4 000 on 16 x 10 needs 44 KB instead of 65) -- and turned into the slab numbers of its columns.
    int cols_used = 0;
    if (live) {
        // the sweep prefetches the codes of the next columns unconditionally: pad both ends
        for (int idx = lane; idx < geo::kGroups * 2 * kCodePad; idx += kWave) {
            const int g = idx / (2 * kCodePad), x = idx - g * (2 * kCodePad);
            const int col = x < kCodePad ? x : F + x;                    // [0, pad) and [F + pad, F + 2 pad)
            unsigned char *dst = refc + g * refc_stride + 2 * col;
            dst[0] = dst[1] = (unsigned char)geo::kZeroSlab;
        }
    }
    if (whole) {
        if (live) stage_span(prof, refs, pair0 * F, pair_end * F, lane);
        if (live && rd_staged) stage_span(prof + rd_off, reads, pair0 * R, pair_end * R, lane);
        __syncthreads();
    }
    constexpr unsigned kZero4 = (unsigned)geo::kZeroSlab * 0x01010101u;
#pragma unroll
    for (int g = 0; g < geo::kGroups; ++g) {
        int pa = 2 * g, pb = 2 * g + 1;
        pa = pa > last ? last : pa;
        pb = pb > last ? last : pb;
        const long long ref_lo = whole ? pair0 * F : (pair0 + pa) * F;
        if (!whole) {
            if (live) stage_span(prof, refs, ref_lo, (pair0 + pb + 1) * F, lane);
            __syncthreads();
        }
        if (live) {
            const int ref_skew = (int)((unsigned long long)(refs + ref_lo) & 15ull);
            const unsigned char *raw_a = prof + ref_skew + (whole ? pa * F : 0), *raw_b = raw_a + (pb - pa) * F;
            unsigned char *codes_g = refc + g * refc_stride + 2 * kCodePad;
            // slab number by class, pair A / pair B of this group: classes 1..4 their slab, 0 and 5..7 the zero slab
            const unsigned slab_a_lo = geo::kZeroSlab | (unsigned)(2 * g) << 8 | (unsigned)(geo::kPairs + 2 * g) << 16 |
                                       (unsigned)(2 * geo::kPairs + 2 * g) << 24;
            const unsigned slab_a_hi = (unsigned)(3 * geo::kPairs + 2 * g) | (kZero4 & 0xFFFFFF00u);
            const unsigned slab_b_lo = slab_a_lo + 0x01010100u, slab_b_hi = slab_a_hi + 1u;
            const int F4 = F & ~3;
            for (int j = 4 * lane; j < F4; j += 4 * kWave) {            // four columns per lane and trip
                const unsigned ca = base_class4(lds_dword_at(raw_a + j)), cb = base_class4(lds_dword_at(raw_b + j));
                const unsigned sa = select_bytes8(slab_a_hi, slab_a_lo, ca), sb = select_bytes8(slab_b_hi, slab_b_lo, cb);
                uint2 codes;                                            // (sa | sb << 8) of columns j, j + 1 | j + 2, j + 3
                codes.x = __builtin_amdgcn_perm(sb, sa, 0x05010400u);
                codes.y = __builtin_amdgcn_perm(sb, sa, 0x07030602u);
                *reinterpret_cast<uint2 *>(codes_g + 2 * j) = codes;
                const unsigned used = (sa ^ kZero4) | (sb ^ kZero4);    // a byte is non-zero where a pair has an ACGT base
                if (used) {
                    const int end = j + 4 - (__builtin_clz(used) >> 3);
                    cols_used = end > cols_used ? end : cols_used;
                }
                if (FIND_BAD) {
                    // "invalid" for the NW end cell: class 0 (Default kernel) or anything but ACGT (SSE kernel)
                    const unsigned bad_a = ~nonzero_bytes(bad_is_non_acgt ? sa ^ kZero4 : ca) & 0x80808080u;
                    const unsigned bad_b = ~nonzero_bytes(bad_is_non_acgt ? sb ^ kZero4 : cb) & 0x80808080u;
                    if (bad_a) atomicMin(&first_bad[2 * (2 * g) + 1], j + (__builtin_ctz(bad_a) >> 3));
                    if (bad_b) atomicMin(&first_bad[2 * (2 * g + 1) + 1], j + (__builtin_ctz(bad_b) >> 3));
                }
            }
            for (int j = F4 + lane; j < F; j += kWave) {                // the rim
                const int ca = base_class(raw_a[j]);
                const int cb = base_class(raw_b[j]);
                const bool va = ca >= 1 && ca <= 4, vb = cb >= 1 && cb <= 4;
                const unsigned sa = va ? (ca - 1) * geo::kPairs + 2 * g : geo::kZeroSlab;
                const unsigned sb = vb ? (cb - 1) * geo::kPairs + 2 * g + 1 : geo::kZeroSlab;
                *reinterpret_cast<unsigned short *>(codes_g + 2 * j) = (unsigned short)(sa | (sb << 8));
                if (va || vb) cols_used = j + 1 > cols_used ? j + 1 : cols_used;
                if (FIND_BAD) {
                    // "invalid" for the NW end cell: class 0 (Default kernel) or anything but ACGT (SSE kernel)
                    if (ca == 0 || (bad_is_non_acgt && ca == 5)) atomicMin(&first_bad[2 * (2 * g) + 1], j);
                    if (cb == 0 || (bad_is_non_acgt && cb == 5)) atomicMin(&first_bad[2 * (2 * g + 1) + 1], j);
                }
            }
        }
        if (!whole) __syncthreads();
    }
    // Staged reads: kPairs * kRows / 4 == 32 K four-row items, K / 2 per lane.  Item `it` holds the classes of padded rows
    // rr .. rr + 3 of pair p (kRows is a multiple of 4: an item never straddles two pairs); (p, rr) walk on by 256 rows
    // per item.  The classes leave the staging area before the barrier, the profile overwrites it after.
    unsigned rd4[K / 2];
    constexpr int kItemPairs = 256 / geo::kRows, kItemRows = 256 % geo::kRows;
    const int item_p0 = (4 * lane) / geo::kRows, item_rr0 = (4 * lane) % geo::kRows, item_q0 = (4 * lane) % K;
    if (live && rd_staged) {
        const unsigned char *raw = prof + rd_off + (int)((unsigned long long)(reads + pair0 * R) & 15ull);
        int p = item_p0, rr = item_rr0;
#pragma unroll
        for (int it = 0; it < K / 2; ++it) {
            const int ps = p > last ? last : p;
            const int pos = row0 + rr;                          // (row0 + kRows == R: pos + 3 < R always)
            const int at = pos < -3 ? -3 : pos;
            unsigned w4 = lds_dword_at(raw + ps * R + at);
            if (pos < 0) w4 = pos < -3 ? 0u : w4 & (0xFFFFFFFFu << (8 * -pos));      // rows before the read: class 0
            rd4[it] = base_class4(w4);
            p += kItemPairs; rr += kItemRows;
            if (rr >= geo::kRows) { rr -= geo::kRows; ++p; }
        }
    }
    if (whole) __syncthreads();

    // ---- query profile: slab[class * kPairs + pair][lane rows] = S(read base of the row, class) ----
    if (live && rd_staged) {
        // scores by class, low and high bytes apart, of slab c: class c + 1 match, the other three of 1..4 mismatch,
        // classes 0 and 5..7 zero_score
        auto table = [&](int c, int shift, unsigned &lo, unsigned &hi) __attribute__((always_inline)) {
            unsigned b[8];
#pragma unroll
            for (int a = 0; a < 8; ++a)
                b[a] = ((unsigned)(unsigned short)(a >= 1 && a <= 4 ? (a == c + 1 ? match : mismatch) : zero_score) >> shift) & 0xFFu;
            lo = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
            hi = b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24;
        };
        int p = item_p0, rr = item_rr0;
#pragma unroll
        for (int it = 0; it < K / 2; ++it) {
            const unsigned cls = rd4[it];
            const int pos = row0 + rr;
            if (FIND_BAD) {
                // a byte of `good` is zero where the row is a read base of class 0 (or, bad_is_non_acgt, of class 5 too)
                unsigned good = bad_is_non_acgt ? select_bytes8(0x00000001u, 0x01010100u, cls) : cls;
                if (pos < 0) good |= pos < -3 ? 0xFFFFFFFFu : ~(0xFFFFFFFFu << (8 * -pos));
                const unsigned bad = ~nonzero_bytes(good) & 0x80808080u;
                if (bad) atomicMin(&first_bad[2 * p], pos + (__builtin_ctz(bad) >> 3));
            }
            // row_key_step: every score of row q of a lane also carries (15 - q) * step (see below)
            u16x2 key01 = u16x2{0, 0}, key23 = u16x2{0, 0};
            if (row_key_step != 0) {
                const int q0 = rr % K, q1 = (rr + 1) % K, q2 = (rr + 2) % K, q3 = (rr + 3) % K;
                key01 = u16x2{(unsigned short)(row_key_step * (15 - q0)), (unsigned short)(row_key_step * (15 - q1))};
                key23 = u16x2{(unsigned short)(row_key_step * (15 - q2)), (unsigned short)(row_key_step * (15 - q3))};
            }
            // row0_score: every score of row 0 of a lane also carries it (score_kernel's tilted sweep: see its hand-over)
            if (row0_score != 0) {
                // rr % K without a division per item: kRows is a multiple of K, so it is (4 lane + 256 it) % K
                int q0 = item_q0 + (256 * it) % K;
                q0 -= q0 >= K ? K : 0;
                // row rr + i of the item is a lane's row 0 where q0 + i is a multiple of K (q0 + i <= K + 2)
                auto row0 = [&](int i) __attribute__((always_inline)) {
                    const int q = q0 + i;
                    return (i == 0 ? q == 0 : q == K) || (K < 4 && q == 2 * K);
                };
                const unsigned short a = (unsigned short)row0_score, none = 0;
                key01 = key01 + u16x2{row0(0) ? a : none, row0(1) ? a : none};
                key23 = key23 + u16x2{row0(2) ? a : none, row0(3) ? a : none};
            }
            unsigned char *dst = prof + p * geo::kPairStride + 2 * rr;          // row_offset(rr / K, rr % K) == 2 rr
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                unsigned lo_lo, lo_hi, hi_lo, hi_hi;
                table(c, 0, lo_lo, lo_hi);
                table(c, 8, hi_lo, hi_hi);
                const unsigned lows = select_bytes8(lo_hi, lo_lo, cls), highs = select_bytes8(hi_hi, hi_lo, cls);
                const u16x2 s01 = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(highs, lows, 0x05010400u)) + key01;
                const u16x2 s23 = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(highs, lows, 0x07030602u)) + key23;
                unsigned *out = reinterpret_cast<unsigned *>(dst + c * geo::kPairs * geo::kPairStride);
                out[0] = __builtin_bit_cast(unsigned, s01);
                out[1] = __builtin_bit_cast(unsigned, s23);
            }
            p += kItemPairs; rr += kItemRows;
            if (rr >= geo::kRows) { rr -= geo::kRows; ++p; }
        }
    }
    if (live && !rd_staged) {
#pragma unroll
        for (int i = 0; i < 2 * K; ++i) {
            const int idx = lane + kWave * i;
            const int p = idx / geo::kRows, rr = idx - p * geo::kRows;
            const int pos = row0 + rr;
            const bool in_read = pos >= 0 && pos < R;
            const int a = in_read ? base_class(rd[i]) : 0;
            if (FIND_BAD && in_read && (a == 0 || (bad_is_non_acgt && a == 5)))
                atomicMin(&first_bad[2 * p], pos);
            const bool valid = a >= 1 && a <= 4;
            const int off = p * geo::kPairStride + geo::row_offset(rr / K, rr % K);
            // row_key_step: every score of row q of a lane also carries (15 - q) * step -- the Smith-Waterman end-cell key
            // of align_fill_tag_kernel<..., PROFKEY>, which then rides on every diagonal candidate for free
            // row0_score: ... and every score of row 0 of a lane that (score_kernel's tilted sweep)
            const short row_key = (short)(row_key_step * (15 - rr % K) + (rr % K == 0 ? row0_score : 0));
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const short sc = (short)((valid ? (a == c + 1 ? match : mismatch) : zero_score) + row_key);
                *reinterpret_cast<short *>(prof + c * geo::kPairs * geo::kPairStride + off) = sc;
            }
        }
    }
    if (live) {
        for (int idx = lane; idx < geo::kPairStride / 4; idx += kWave) {          // dword idx: rows 2 idx, 2 idx + 1
            const unsigned lo = (unsigned short)(zero_score + row_key_step * (15 - (2 * idx) % K) + ((2 * idx) % K == 0 ? row0_score : 0));
            const unsigned hi = (unsigned short)(zero_score + row_key_step * (15 - (2 * idx + 1) % K) + ((2 * idx + 1) % K == 0 ? row0_score : 0));
            reinterpret_cast<unsigned *>(prof + geo::kZeroSlab * geo::kPairStride)[idx] = lo | (hi << 16);
        }
    }
    __syncthreads();
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const int other = __shfl_xor(cols_used, d, kWave);
        cols_used = other > cols_used ? other : cols_used;
    }
    w.cols_used = __builtin_amdgcn_readfirstlane(cols_used);
    w.prof = prof;
    w.refc = refc + 2 * kCodePad;          // entry of column 0
    w.first_bad = first_bad;
    w.pair0 = pair0;
    w.last = last;
    return live;
}

// ---- row tables: the set-up of score_kernel<G, K, kAlgSW, kGapAffineSym>'s tilted sweep where every score fits a byte ----
// (cell_rules.h: sym_affine_row_tables_ok).  No profile is built.  Each lane keeps, for its K rows, one dword per row and
// pair -- Ta[q], Tb[q]: byte c the score of the row's read base against reference class c + 1 (match or mismatch; all four
// zero_score where the row is a padding row or the base no ACGT; EVERY row plus row0_score, the o - x its diagonal is short
// of: the step reads it from H - (o - x) in every row, as row 0 always did) -- and the references
// become a stream of SELECTOR dwords, one per column and lane group: bytes {ca, 0x0c, 4 + cb, 0x0c}, ca / cb the class - 1
// of pair A's / pair B's base, so that v_perm_b32(Tb[q], Ta[q], selector) IS the packed score of row q (selector byte 0x0c
// yields 0x00: the high bytes).  A base that is no ACGT, and every column of the pads, selects 0x0c in its half too: the
// score 0 where the profile has zero_score.  score_kernel says why that is exact outside a reference's ACGT columns;
// `repair` comes back true (wave-uniform) where some pair of the wave has such a base BEFORE its last ACGT base.
// LDS of a wave (row_table_lds): the wave's raw references, then the stream, row_table_pad(G) pad columns at either end of
// every group's; the raw reads are staged where the stream is built once they have been read.
// THE COMPACT STREAM (8 x 19 only: tilt_tables_only).  That tile holds 16 pairs per wave and runs two 4-wave blocks per CU or not
// at all, so its stream is 16 bits per column and group -- {ca, 4 + cb}, the two bytes of the selector that carry anything -- and
// the sweep widens each entry with one v_perm_b32 against kSelZero4 (row_table_lds16 has the sizes).  Everything else here -- the
// tables, the pads, `repair` -- is the same; the rows of a lane are still looked up four at a time, and the group of four that
// holds row 16 .. 18 reads one base past the lane's rows and drops it.
constexpr int row_table_pad(int G) { return G + 4; }       // columns -(G - 1) .. F + G are read (the sweep, two steps of prefetch)
constexpr unsigned kSelZero4 = 0x0c0c0c0cu;
constexpr unsigned kSelWiden = 0x04010400u;                // v_perm_b32(kSelZero4, {ca, 4 + cb, -, -}, .) = {ca, 0x0c, 4 + cb, 0x0c}

template <int G, int K>
__device__ __forceinline__ bool wave_setup_tables(const uint8_t *reads, const uint8_t *refs, long long n, int R, int F,
                                                  int refs_area, int sel_stride, int wave_lds, short match, short mismatch,
                                                  short zero_score, short row0_score, unsigned block, WaveTables &w,
                                                  unsigned (&Ta)[K], unsigned (&Tb)[K], bool &repair) {
    using geo = Geo<G, K>;
    constexpr int kPad = row_table_pad(G);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const int row0 = R - geo::kRows;                     // read position of padded row 0 (one sweep covers the read)

    unsigned char *raw = valign_smem + (size_t)wave * wave_lds;
    unsigned char *sel = raw + refs_area;

    const int waves = blockDim.x / kWave;
    const long long pair0 = ((long long)block * waves + wave) * geo::kPairs;
    const bool live = pair0 < n;
    long long pair_end = pair0 + geo::kPairs;
    if (pair_end > n) pair_end = n;
    const int last = (int)(pair_end - pair0) - 1;

    if (live) {
        stage_span(raw, refs, pair0 * F, pair_end * F, lane);
        stage_span(sel, reads, pair0 * R, pair_end * R, lane);
    }
    __syncthreads();

    // ---- the lane's 2K rows: four read bases at a time to their classes, the classes to the four score bytes of each row ----
    if (live) {
        // byte a of {hi, lo}: the score of a read base of class a against reference class c + 1
        auto table = [&](int c, unsigned &lo, unsigned &hi) __attribute__((always_inline)) {
            unsigned b[8];
#pragma unroll
            for (int a = 0; a < 8; ++a) b[a] = (unsigned)(a >= 1 && a <= 4 ? (a == c + 1 ? match : mismatch) : zero_score) & 0xFFu;
            lo = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
            hi = b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24;
        };
        unsigned t_lo[4], t_hi[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) table(c, t_lo[c], t_hi[c]);
        const unsigned char *raw_rd = sel + (int)((unsigned long long)(reads + pair0 * R) & 15ull);
        using lmap = LaneMap<G, score_lane_stride(G, K)>;               // (the rows a lane loads follow its place in the group)
        const int grp = lmap::kInterleaved ? lmap::grp(lane) : lane / G, l = lmap::kInterleaved ? lmap::l(lane) : lane % G;   // (score_kernel says why both)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            int p = 2 * grp + half;
            p = p > last ? last : p;
#pragma unroll
            for (int q0 = 0; q0 < K; q0 += 4) {
                const int pos = row0 + l * K + q0;
                const int at = pos < -3 ? -3 : pos;
                unsigned w4 = lds_dword_at(raw_rd + p * R + at);
                if (pos < 0) w4 = pos < -3 ? 0u : w4 & (0xFFFFFFFFu << (8 * -pos));      // rows before the read: class 0
                const unsigned cls = base_class4(w4);
                unsigned col[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) col[c] = select_bytes8(t_hi[c], t_lo[c], cls);   // byte i: row q0 + i against class c + 1
                const unsigned lo01 = __builtin_amdgcn_perm(col[1], col[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(col[1], col[0], 0x07030602u);
                const unsigned lo23 = __builtin_amdgcn_perm(col[3], col[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(col[3], col[2], 0x07030602u);
                unsigned (&T)[K] = half ? Tb : Ta;
                T[q0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
                if constexpr (K % 2 == 0) {
                    T[q0 + 1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
                    if (q0 + 2 < K) {
                        T[q0 + 2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
                        T[q0 + 3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
                    }
                } else {                                    // (odd K: the last group of four has one or three rows)
                    if (q0 + 1 < K) T[q0 + 1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
                    if (q0 + 2 < K) T[q0 + 2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
                    if (q0 + 3 < K) T[q0 + 3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
                }
            }
        }
        const unsigned r4 = ((unsigned)row0_score & 0xFFu) * 0x01010101u;      // (no byte carries: the rule bounds every sum by 255)
#pragma unroll
        for (int q = 0; q < K; ++q) {                                          // every row: the step takes its diagonals from H - (o - x)
            Ta[q] += r4;
            Tb[q] += r4;
        }
    }
    __syncthreads();                                                           // the raw reads make way for the stream

    // ---- the selector stream ----
    int cols_used = 0;
    bool before_last = false;
    unsigned *stream = reinterpret_cast<unsigned *>(sel);
    const int stride_dw = sel_stride / 4;
    constexpr bool SEL16 = tilt_tables_only(G, K);                   // the compact stream: 16 bits per column and group
    unsigned short *stream16 = reinterpret_cast<unsigned short *>(sel);
    const int stride_h = sel_stride / 2;
    if (live) {
        for (int idx = lane; idx < geo::kGroups * 2 * kPad; idx += kWave) {
            const int g = idx / (2 * kPad), x = idx - g * (2 * kPad);
            if constexpr (SEL16) stream16[g * stride_h + (x < kPad ? x : F + x)] = (unsigned short)0x0c0c;
            else stream[g * stride_dw + (x < kPad ? x : F + x)] = kSelZero4;     // [0, pad) and [F + pad, F + 2 pad)
        }
        const int ref_skew = (int)((unsigned long long)(refs + pair0 * F) & 15ull);
        typedef unsigned short u16;
#pragma unroll
        for (int g = 0; g < geo::kGroups; ++g) {
            int pa = 2 * g, pb = 2 * g + 1;
            pa = pa > last ? last : pa;
            pb = pb > last ? last : pb;
            const unsigned char *raw_a = raw + ref_skew + pa * F, *raw_b = raw + ref_skew + pb * F;
            unsigned *out_g = stream + g * stride_dw + kPad;
            unsigned short *out16_g = stream16 + g * stride_h + kPad;           // (8-byte aligned: the stride and the pad are)
            // per pair: {1 + its last ACGT column, 0xFFFF - its first column that is none} -- one packed maximum each
            u16x2 ends_a = u16x2{0, 0}, ends_b = u16x2{0, 0};
            auto note = [](u16x2 &ends, unsigned acgt, int j) __attribute__((always_inline)) {     // acgt: a byte is non-zero where the column has an ACGT base
                const unsigned none = ~nonzero_bytes(acgt) & 0x80808080u;
                const u16 end = acgt ? (u16)(j + 4 - (__builtin_clz(acgt) >> 3)) : (u16)0;
                const u16 first_none = none ? (u16)(0xFFFF - (j + (__builtin_ctz(none) >> 3))) : (u16)0;
                ends = __builtin_elementwise_max(ends, u16x2{end, first_none});
            };
            const int F4 = F & ~3;
            for (int j = 4 * lane; j < F4; j += 4 * kWave) {                    // four columns per lane and trip
                const unsigned ca = base_class4(lds_dword_at(raw_a + j)), cb = base_class4(lds_dword_at(raw_b + j));
                // selector by class: 1..4 the table byte (pair B: of the second table), 0 and 5..7 the constant zero
                const unsigned sa = select_bytes8(0x0c0c0c03u, 0x0201000cu, ca), sb = select_bytes8(0x0c0c0c07u, 0x0605040cu, cb);
                if constexpr (SEL16) {
                    uint2 s;                                                    // (sa | sb << 8) of columns j, j + 1 | j + 2, j + 3
                    s.x = __builtin_amdgcn_perm(sb, sa, 0x05010400u);
                    s.y = __builtin_amdgcn_perm(sb, sa, 0x07030602u);
                    *reinterpret_cast<uint2 *>(out16_g + j) = s;
                } else {
                    uint4 s;
                    s.x = __builtin_amdgcn_perm(sb, sa, 0x0c040c00u) | 0x0c000c00u;
                    s.y = __builtin_amdgcn_perm(sb, sa, 0x0c050c01u) | 0x0c000c00u;
                    s.z = __builtin_amdgcn_perm(sb, sa, 0x0c060c02u) | 0x0c000c00u;
                    s.w = __builtin_amdgcn_perm(sb, sa, 0x0c070c03u) | 0x0c000c00u;
                    *reinterpret_cast<uint4 *>(out_g + j) = s;
                }
                note(ends_a, sa ^ kSelZero4, j);
                note(ends_b, sb ^ kSelZero4, j);
            }
            for (int j = F4 + lane; j < F; j += kWave) {                        // the rim
                const int ca = base_class(raw_a[j]), cb = base_class(raw_b[j]);
                const bool va = ca >= 1 && ca <= 4, vb = cb >= 1 && cb <= 4;
                if constexpr (SEL16) out16_g[j] = (unsigned short)((va ? (unsigned)(ca - 1) : 0x0cu) | (vb ? (unsigned)(cb + 3) : 0x0cu) << 8);
                else out_g[j] = (va ? (unsigned)(ca - 1) : 0x0cu) | (vb ? (unsigned)(cb + 3) : 0x0cu) << 16 | 0x0c000c00u;
                ends_a = __builtin_elementwise_max(ends_a, u16x2{va ? (u16)(j + 1) : (u16)0, va ? (u16)0 : (u16)(0xFFFF - j)});
                ends_b = __builtin_elementwise_max(ends_b, u16x2{vb ? (u16)(j + 1) : (u16)0, vb ? (u16)0 : (u16)(0xFFFF - j)});
            }
#pragma unroll
            for (int d = kWave / 2; d >= 1; d >>= 1) {
                ends_a = __builtin_elementwise_max(ends_a, __builtin_bit_cast(u16x2, __shfl_xor(__builtin_bit_cast(int, ends_a), d, kWave)));
                ends_b = __builtin_elementwise_max(ends_b, __builtin_bit_cast(u16x2, __shfl_xor(__builtin_bit_cast(int, ends_b), d, kWave)));
            }
            before_last |= 0xFFFF - (int)ends_a.y < (int)ends_a.x || 0xFFFF - (int)ends_b.y < (int)ends_b.x;
            cols_used = (int)ends_a.x > cols_used ? (int)ends_a.x : cols_used;
            cols_used = (int)ends_b.x > cols_used ? (int)ends_b.x : cols_used;
        }
    }
    __syncthreads();
    repair = __builtin_amdgcn_readfirstlane((int)before_last) != 0;
    w.cols_used = __builtin_amdgcn_readfirstlane(cols_used);
    w.prof = raw;
    w.refc = SEL16 ? reinterpret_cast<unsigned char *>(stream16 + kPad) : reinterpret_cast<unsigned char *>(stream + kPad);          // entry of column 0 of the first group
    w.first_bad = nullptr;
    w.pair0 = pair0;
    w.last = last;
    return live;
}

// K/2 dwords starting at LDS byte offset `addr`, with the widest loads the lane stride allows
template <int K>
__device__ __forceinline__ void lds_load_lane(unsigned addr, unsigned (&v)[K / 2]) {
    constexpr int N = K / 2;
    if constexpr ((K * 2) % 16 == 0) {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) {
            const u32x4 x = *(lds_cu32x4 *)(addr + 16 * i);
            v[4 * i] = x.x; v[4 * i + 1] = x.y; v[4 * i + 2] = x.z; v[4 * i + 3] = x.w;
        }
    } else if constexpr ((K * 2) % 8 == 0) {
#pragma unroll
        for (int i = 0; i < N / 2; ++i) {
            const u32x2 x = *(lds_cu32x2 *)(addr + 8 * i);
            v[2 * i] = x.x; v[2 * i + 1] = x.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = *(lds_cu32 *)(addr + 4 * i);
    }
}

// S[q] (q = 0..K-1) from the raw profile dwords of pair A (low halves) and pair B (high halves)
template <int K>
__device__ __forceinline__ void merge_profile(const unsigned (&va)[K / 2], const unsigned (&vb)[K / 2], s16x2 (&S)[K]) {
#pragma unroll
    for (int c = 0; c < K / 2; ++c) {
        S[2 * c + 0] = as_pk(__builtin_amdgcn_perm(vb[c], va[c], 0x05040100u));
        S[2 * c + 1] = as_pk(__builtin_amdgcn_perm(vb[c], va[c], 0x07060302u));
    }
}

// S[q] (q = 0..K-1): substitution scores of this lane's K rows against the current reference
// bases of pair A (low halves) and pair B (high halves), from the LDS profile.
template <int G, int K>
__device__ __forceinline__ void fetch_profile(unsigned addr_a, unsigned addr_b, s16x2 (&S)[K]) {
    unsigned va[K / 2], vb[K / 2];
    lds_load_lane<K>(addr_a, va);
    lds_load_lane<K>(addr_b, vb);
    merge_profile<K>(va, vb, S);
}

// (Round 2 also tried fetching the profile WITHOUT the merge instruction -- ds_read_u16_d16 / _d16_hi straight into the
// register halves, which removes the v_perm_b32 per register (hot loop 217 -> 197 VALU per step pair, int16 affine): 2K
// narrow LDS returns per step instead of ~K/2 wide ones cost more than the 10 % VALU they save -- int16 affine 13.10 ->
// 13.54 ms, half-float affine 11.47 -> 12.14 ms, linear 7.19 -> 8.66 ms: every LDS return writes a full wave of VGPRs
// whatever its width.  The code is gone; DESIGN.md section 3 keeps the numbers.)

// GAPS selects the recurrence (the constants: cell_constants.h): kGapLinear (two gap scores), kGapSym (linear with
// gap_read == gap_ref: one subtract serves both neighbours), kGapAffine (Gotoh extension), kGapAffineSym (affine with
// open_read == open_ref and ext_read == ext_ref).
// kGapAffineSymF16: the same recurrence as kGapAffineSym on packed half floats: every value is an
// integer of magnitude <= 2048, which fp16 represents exactly, and gfx950's v_pk_maximum3_f16
// takes three operands -- h = max3(diag + S, E, F), E = max3(E - ext, H - open, 0) (which floors the
// whole SW cell at zero) and the SW maximum tracking two rows at a time: 8.5 instead of 10 packed
// instructions per register (NW variant, tilted frame: 6 instead of 7, gap matrices start at a real -inf).  The
// engine picks it when shape x scoring stays inside +-2048.
// kGapAffineF16: half floats with four different open / extend scores: 9.5 instead of 11
// kGapSymF16: linear gaps with gap_read == gap_ref on half floats.  NW variant: h = max3(diag + S', left, up) in the tilted
// frame (score_kernel) -- perm, add, max3: 3 packed instructions per register.  Smith-Waterman needs the zero
// floor: there every value is scaled by 2^-10 (exact for integers below 1024), which turns the floor into the
// hardware clamp of v_pk_add_f16 -- max(h + g, 0) is ONE instruction, and a register pair (h, max(h + g, 0))
// per cell gives h = max3(diag + S, left', up'), left' / up' being the clamped registers: 4 per register.

constexpr int kTrackAll = 0, kTrackNone = 1, kTrackPair = 2;   // see score_kernel's step

// Half-float NW kernels: the constant their tilted frame is centred by -- half of the largest value a cell of the
// frame can take (best possible score plus what row and column add at the far corner).
__host__ __device__ inline int nw_frame_centre(int R, int F, int rows, int match, int mismatch, int tilt_row, int tilt_col) {
    const int best = match > mismatch ? match : mismatch;
    const int top = (R < F ? R : F) * (best > 0 ? best : 0);
    return (top + tilt_row * (rows + 1) + tilt_col * (F + 1)) / 2;
}

template <int G, int K, int ALG, int GAPS>
__global__ void __launch_bounds__(256)
score_kernel(const ScoreArgs args) {
    using geo = Geo<G, K>;
    constexpr bool F16 = GAPS == kGapAffineSymF16 || GAPS == kGapAffineF16;
    constexpr bool F16SYM = GAPS == kGapAffineSymF16;
    constexpr bool AFFINE = GAPS == kGapAffine || GAPS == kGapAffineSym || F16;
    constexpr bool SYM = GAPS == kGapSym;
    constexpr bool LINF16 = GAPS == kGapSymF16;
    constexpr bool AFFSYM = GAPS == kGapAffineSym;
    constexpr bool SOURCES = AFFSYM && ALG == kAlgSW;      // int16 symmetric affine SW carries gap sources (see the step)
    const int lane = threadIdx.x & (kWave - 1);
    // lane -> (group, lane of the group): contiguous, but for the 8 x 19 tile, whose two groups of a DPP row interleave (lane_map.h)
    using lmap = LaneMap<G, score_lane_stride(G, K)>;
    // (The contiguous map stays written out here: taken through the map's functions the same arithmetic reaches the compiler in
    // another order, and every contiguous instance -- 168 score kernels -- comes out an instruction or two different from the
    // code it has had.  The static_assert ties the two; tests/lane_map_check.cpp checks the map lane by lane.)
    static_assert(lmap::kInterleaved || (lmap::grp(kWave - 3) == (kWave - 3) / G && lmap::l(kWave - 3) == (kWave - 3) % G), "the contiguous map is lane / G, lane % G");
    const int grp = lmap::kInterleaved ? lmap::grp(lane) : lane / G;
    const int l = lmap::kInterleaved ? lmap::l(lane) : lane % G;

    // the batch (or, in a length-sorted launch, the group this block belongs to): wave-uniform
    const uint8_t *reads = args.reads, *refs = args.refs;
    int16_t *scores = args.scores;
    long long n_pairs = args.n;
    int F_batch = args.F;
    unsigned block = blockIdx.x;
    if (args.n_groups > 0) {
        int g = 0;
        while (g + 1 < args.n_groups && block >= args.groups[g].block_end) ++g;
        block -= g ? args.groups[g - 1].block_end : 0u;
        reads += args.groups[g].read_ofs;
        refs += args.groups[g].ref_ofs;
        scores += args.groups[g].pair_ofs;
        n_pairs = args.groups[g].n;
        F_batch = args.groups[g].F;
    }

    WaveTables w;
    // the query profile holds the substitution scores in the cell format of the recurrence
    // (kGapSymF16: S - g, also for the rows / bases that score 0)
    // (kGapSymF16: NW S - g, also for the rows / bases that score 0; SW S * 2^-10)
    constexpr bool LINF16_SW = LINF16 && ALG == kAlgSW, LINF16_NW = LINF16 && ALG == kAlgNW;
    // The NW variant (no zero floor) runs in a tilted frame: cell (p, j) -- p padded row, j matrix column -- is kept as
    //   V'(p, j) = V(p, j) - g_ref * p - g_read * j          (g: the gap score, or the extension score with affine gaps)
    // In it a gap step (an extension) costs nothing -- "up + g" and "left + g" are simply the neighbours' registers,
    // E' = max(E', H' + open - ext), F' likewise -- and the diagonal step pays both, folded into the query profile
    // (S - g_ref - g_read, also for the rows / bases that score 0).  One or two packed instructions per register less in
    // every recurrence; results are taken out of the frame where they are read (last row: per step, last column: once).
    constexpr bool TILT = ALG == kAlgNW;
    constexpr bool HALF = F16 || LINF16;          // cells are half floats (bit patterns in the s16x2 containers)
    const int tilt_row = TILT ? -(int)(AFFINE ? args.ext_ref : args.gap_ref) : 0;
    const int tilt_col = TILT ? -(int)(AFFINE ? args.ext_read : args.gap_read) : 0;
    int fold = tilt_row + tilt_col;
    // (int16 symmetric affine Smith-Waterman in its tilted biased form -- see the sweep below -- pays both extensions on the
    // diagonal as the NW frame does: 2x on every score of the profile, the zero slab included)
    // (... and its lanes hand H - (o - x) of their last row down, so every score of a lane's row 0 carries the o - x back)
    short s_row0 = 0;
    // TILT_BUILT: the instance carries the tilted biased form; TABLES_ONLY (8 x 19): that form with the row tables and nothing else --
    // no LDS profile, no plain biased form, no gap-source form: a launch without the row-table bits does nothing
    constexpr bool TILT_BUILT = SOURCES && tilt_frame_built(G, K), TABLES_ONLY = SOURCES && tilt_tables_only(G, K);
    if constexpr (TILT_BUILT) {
        if (args.sym_max3_bias > 0 && (args.sym_max3_bias >> 16) != 0) {
            fold = -2 * (int)args.ext_ref;
            s_row0 = (short)((int)args.ext_ref - (int)args.open_ref);
        }
    }
    // Half-float cells are exact up to 2048 in magnitude and the frame only ever adds: a constant taken off every cell
    // (borders start at -centre, results get it back) puts the sweep's value range [~0, top + tilt] around zero.  The
    // host checks the range with the same formula (Engine::half_float_exact).
    const int centre = (HALF && TILT) ? nw_frame_centre(args.R, F_batch, G * K, args.match, args.mismatch, tilt_row, tilt_col) : 0;
    // ... and results are collected as "value - half the best possible score": what is taken off a cell on its way out
    // of the frame, tilt - centre + rcentre, lies within +- half the frame's tilt and the difference within +- rcentre --
    // every constant and every intermediate exact
    const int rcentre = (HALF && TILT) ? nw_frame_centre(args.R, F_batch, G * K, args.match, args.mismatch, 0, 0) : 0;
    const float unit = LINF16_SW ? 1.0f / 1024.0f : 1.0f;
    auto cell = [](int v) __attribute__((always_inline)) {           // an integer in the cell format of this kernel, both halves
        return HALF ? pk(__builtin_bit_cast(short, (_Float16)v)) : pk((short)v);
    };
    auto cell_add = [](s16x2 a, s16x2 b) __attribute__((always_inline)) {
        return HALF ? __builtin_bit_cast(s16x2, __builtin_bit_cast(f16x2, a) + __builtin_bit_cast(f16x2, b)) : a + b;
    };
    auto cell_sub = [](s16x2 a, s16x2 b) __attribute__((always_inline)) {
        return HALF ? __builtin_bit_cast(s16x2, __builtin_bit_cast(f16x2, a) - __builtin_bit_cast(f16x2, b)) : a - b;
    };
    const short s_match = HALF ? __builtin_bit_cast(short, (_Float16)(((int)args.match + fold) * unit)) : (short)(args.match + fold);
    const short s_mismatch = HALF ? __builtin_bit_cast(short, (_Float16)(((int)args.mismatch + fold) * unit)) : (short)(args.mismatch + fold);
    const short s_zero = HALF ? __builtin_bit_cast(short, (_Float16)fold) : (short)fold;
    // (... and where every such score fits a byte -- bit 17, sym_affine_row_tables_ok -- the scores of a lane's rows stay in
    // registers and no profile is built: wave_setup_tables)
    bool tables = false, repair = false;
    unsigned Ta[K], Tb[K];
    if constexpr (TABLES_ONLY) {
        tables = args.sym_max3_bias > 0 && (args.sym_max3_bias >> 16 & 3) == 3;
        if (!tables) return;                   // (wave-uniform, before any barrier)
        if (!wave_setup_tables<G, K>(reads, refs, n_pairs, args.R, F_batch, args.prof_area, args.refc_stride, args.wave_lds,
                                     s_match, s_mismatch, s_zero, s_row0, block, w, Ta, Tb, repair))
            return;
        // which form this wave runs, once per wave: a plain store of 1 (every wave that writes a word writes the same value)
        if (args.form_seen != nullptr && lane == 0) args.form_seen[repair ? 1 : 0] = 1u;
    } else if constexpr (TILT_BUILT) {
        tables = args.sym_max3_bias > 0 && (args.sym_max3_bias >> 16 & 3) == 3;
        bool live = false;
        if (tables)
            live = wave_setup_tables<G, K>(reads, refs, n_pairs, args.R, F_batch, args.prof_area, args.refc_stride, args.wave_lds,
                                           s_match, s_mismatch, s_zero, s_row0, block, w, Ta, Tb, repair);
        if (!tables)
            live = wave_setup<G, K, false>(reads, refs, n_pairs, args.R, F_batch, args.prof_area, args.refc_stride,
                                           args.wave_lds, s_match, s_mismatch, w, false, block, s_zero, kOneSweep, 0, s_row0);
        if (!live) return;
    } else if (!wave_setup<G, K, false>(reads, refs, n_pairs, args.R, F_batch, args.prof_area, args.refc_stride,
                                        args.wave_lds, s_match, s_mismatch, w, false, block, s_zero, kOneSweep, 0, s_row0))
        return;
    const long long pair0 = w.pair0;
    // Smith-Waterman: columns after the last ACGT base of every reference in the wave (the NUL
    // padding of ragged batches) score nothing and can never raise the maximum -- not swept.
    // The NW variant's result lives in the last column and row of the PADDED matrix: full sweep.
    const int F = (ALG == kAlgSW) ? w.cols_used : F_batch;

    // ---- per-lane constants (LDS byte offsets) ----
    const unsigned lmask = l == 0 ? 0u : 0xFFFFFFFFu;            // group leader: row-0 border
    const unsigned lane_base = lds_offset(w.prof) + l * geo::kLaneBytes;     // + slab * kPairStride
    // Smith-Waterman starts the sweep at the first lane that owns a row of the read: the `lead` lanes above it hold
    // padding rows only, whose cells are zero at every column, so every lane simply works `lead` columns further right
    // (lane l at step t: column t - l + lead) and the sweep is `lead` steps shorter.
    const int lead = (ALG == kAlgSW && G * K > args.R) ? (G * K - args.R) / K : 0;
    unsigned code_addr = lds_offset(w.refc) + grp * args.refc_stride - 2 * (l - lead);   // + 2 per step

    s16x2 g_read, g_ref, o_read, e_read, o_ref, e_ref;
    if (ALG == kAlgSW) {           // magnitudes for the unsigned floor-at-zero subtract
        g_read = pk((short)-args.gap_read);   g_ref = pk((short)-args.gap_ref);
        o_read = pk((short)-args.open_read);  e_read = pk((short)-args.ext_read);
        o_ref = pk((short)-args.open_ref);    e_ref = pk((short)-args.ext_ref);
    } else {                       // tilted frame: gap steps / extensions are free, an opening costs open - extend
        g_read = g_ref = e_read = e_ref = pk(0);
        o_read = pk((short)(args.open_read - args.ext_read));
        o_ref = pk((short)(args.open_ref - args.ext_ref));
    }
    // gap matrices start at minus infinity in the NW variant (half floats have the real thing: 0xFC00)
    const s16x2 border_f = pk(ALG == kAlgNW ? (F16 ? (short)0xFC00 : kNegInf) : (short)0);
    // half-float recurrence: signed addends (open, extend <= 0)
    const _Float16 open_h = (_Float16)(int)(TILT ? args.open_ref - args.ext_ref : args.open_ref), ext_h = (_Float16)(int)args.ext_ref;
    const _Float16 open_rd = (_Float16)(int)(TILT ? args.open_read - args.ext_read : args.open_read), ext_rd = (_Float16)(int)args.ext_read;
    const f16x2 o_half = f16x2{open_h, open_h}, e_half = f16x2{ext_h, ext_h}, zero_half = f16x2{(_Float16)0, (_Float16)0};
    const f16x2 o_read_half = f16x2{open_rd, open_rd}, e_read_half = f16x2{ext_rd, ext_rd};

    // Hl: H of the previous column; El: E of the previous column; HOl (symmetric affine, NW variant and half floats):
    // H - open of the previous column, which feeds E of this column (and, within a column, F of
    // the next row), so the subtract is done once per cell instead of twice.  Int16 symmetric affine Smith-Waterman
    // (SOURCES) keeps the best gap SOURCE of the row in El instead and has no HOl.
    s16x2 Hl[K], El[K], HOl[K];
#pragma unroll
    for (int q = 0; q < K; ++q) {
        Hl[q] = cell(tilt_row * (l * K + q) - centre);          // column 0: the zero border (in the NW frame: what the row adds)
        El[q] = border_f;
        // border H plus (SW: minus) open
        HOl[q] = (ALG == kAlgSW) ? pk(0) : (F16 ? cell_add(Hl[q], pk(__builtin_bit_cast(short, open_h))) : Hl[q] + o_ref);
    }
    s16x2 up0 = pk(0), h_last = Hl[K - 1], f_last = border_f, best = pk(0);
    s16x2 fup_keep = border_f;       // NW variant, 16-lane groups: F of the row above the lane's rows (see the step)
    // NW result: max(0, last row, last column) -- kept as "value - centre" (half floats: the sum itself may not be exact)
    s16x2 row_best = cell(-rcentre);
    int j = -l;                                                  // this lane's column at step t
    // NW frame: the all-zero row above padded row 0, as the group leader sees it (row -1, column 1 at step 0, one
    // column on per step), and what the last padded row adds at this lane's column (taken off before the row maximum)
    s16x2 top_row = pk(0), top_step = pk(0), row_tilt = pk(0);
    const s16x2 col_step = cell(tilt_col);
    if (TILT) {
        if (l == 0) {
            top_row = cell(-tilt_row + tilt_col - centre);
            top_step = col_step;                       // (stays zero in the other lanes: it is OR-ed into their row above)
            up0 = cell(-tilt_row - centre);            // row -1, column 0: the diagonal of the first cell
        }
        row_tilt = cell(tilt_row * (G * K - 1) + tilt_col * (1 - l) - centre + rcentre);
    }

    // LDS fetches run one step ahead of the arithmetic (every lane, every step: the code arrays are
    // padded): on entry to step t the raw profile dwords of step t and the slab numbers of step t+1
    // are already in registers, so no step waits for its own LDS round trips (+3 % at 16x10, +12 %
    // at one wave per SIMD).
    constexpr bool PIPE = true;
    unsigned pa[K / 2], pb[K / 2];
    s16x2 S0[K], S1[K];          // the scores of a step (two buffers: the steady loop takes two steps per trip)
    unsigned ca_next = 0, cb_next = 0;
    if constexpr (!TABLES_ONLY) if (PIPE && !tables) {          // (the row-table sweep has no profile and fetches its own stream)
        const unsigned ca = *(lds_cu8 *)(code_addr), cb = *(lds_cu8 *)(code_addr + 1);
        lds_load_lane<K>(lane_base + ca * geo::kPairStride, pa);
        lds_load_lane<K>(lane_base + cb * geo::kPairStride, pb);
        ca_next = *(lds_cu8 *)(code_addr + 2);
        cb_next = *(lds_cu8 *)(code_addr + 3);
    }

    // The kernel with two steady loops (SOURCES) walks the code array with a pointer, so that each loop's addressing is worked
    // out from LDS address uses (one add per trip, the four prefetch offsets in the instructions) whichever loop it is
    lds_cu8 *code_ptr = (lds_cu8 *)code_addr;

    // One step of the skewed sweep.  MASKED steps (NW variant only) EXEC-mask lanes whose column is outside
    // [0, F) (pipeline fill and drain); in the steady phase every lane is inside.
    // TRACK selects how a step feeds the running SW maximum: kTrackAll = every diag+S of the step;
    // in the steady phase of the shared-gap kernel steps go in pairs -- the first adds nothing
    // (kTrackNone), the second adds every max(left, up) plus its last row (kTrackPair): the "left"s
    // are all cells of the first step, the "up"s all cells of the second but the last row.  K + 1
    // maxima per two steps instead of 2K.  The gap-source form of symmetric affine Smith-Waterman (SOURCES) does the
    // same with its max(XE, XF).
    auto step = [&](auto masked_tag, auto track_tag, s16x2 (&S)[K], s16x2 (&Snext)[K]) __attribute__((always_inline)) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        constexpr int TRACK = decltype(track_tag)::value;
        const s16x2 diag0 = up0;
        if (G == 16) {             // row_shr:1 is exactly "previous lane of my 16-lane group, else 0"
            up0 = as_pk((unsigned)__builtin_amdgcn_update_dpp(0, (int)as_u32(h_last), 0x111, 0xF, 0xF, true));
        } else {
            up0 = as_pk(from_prev_lane(as_u32(h_last)) & lmask);
        }
        if (TILT) up0 = as_pk(as_u32(up0) | as_u32(top_row));         // (zero in every lane but the group leader)
        s16x2 fup0 = border_f;
        if (AFFINE && !SOURCES) {          // (the gap-source form fetches its own, behind its first diag + S)
            if (G == 16 && ALG == kAlgSW) {      // (row_shr:1: the group's first lane reads 0, the Smith-Waterman border)
                fup0 = as_pk((unsigned)__builtin_amdgcn_update_dpp(0, (int)as_u32(f_last), 0x111, 0xF, 0xF, true));
            } else if (G != 16) {
                const unsigned fv = from_prev_lane(as_u32(f_last));
                fup0 = (ALG == kAlgNW) ? as_pk(l == 0 ? as_u32(border_f) : fv) : as_pk(fv & lmask);
            }
            if (G == 16 && ALG == kAlgNW) {      // the group's first lane keeps what the register held: the border, for good
                fup_keep = as_pk((unsigned)__builtin_amdgcn_update_dpp((int)as_u32(fup_keep), (int)as_u32(f_last), 0x111, 0xF, 0xF, false));
                fup0 = fup_keep;
            }
        }
        s16x2 gup0 = pk(0);        // kGapSymF16 (SW): max(h + g, 0) of the row above
        if (LINF16_SW) gup0 = as_pk(group_prev_or_zero<G>(as_u32(f_last), lmask));
        if (PIPE) {
            merge_profile<K>(pa, pb, S);                                     // step t's scores
            lds_load_lane<K>(lane_base + ca_next * geo::kPairStride, pa);     // step t+1's profile rows
            lds_load_lane<K>(lane_base + cb_next * geo::kPairStride, pb);
            if constexpr (SOURCES) {
                ca_next = code_ptr[4];
                cb_next = code_ptr[5];
            } else {
                ca_next = *(lds_cu8 *)(code_addr + 4);                        // step t+2's slab numbers
                cb_next = *(lds_cu8 *)(code_addr + 5);
            }
        }
        if (!MASKED || (unsigned)j < (unsigned)F) {
            if (!PIPE) {
                const unsigned ca = *(lds_cu8 *)(code_addr), cb = *(lds_cu8 *)(code_addr + 1);
                fetch_profile<G, K>(lane_base + ca * geo::kPairStride, lane_base + cb * geo::kPairStride, S);
            }
            if (LINF16_SW) {
                // h = max3(diag + S, left', up') with x' = max(x + g, 0) kept beside x (El[] holds the x');
                // everything times 2^-10, so the floor is the clamp of the packed add
                auto hf = [](s16x2 v) __attribute__((always_inline)) { return __builtin_bit_cast(f16x2, v); };
                auto bits = [](f16x2 v) __attribute__((always_inline)) { return __builtin_bit_cast(s16x2, v); };
                const _Float16 gs = (_Float16)((int)args.gap_ref * (1.0f / 1024.0f));
                const f16x2 g_unit = f16x2{gs, gs}, zero2 = f16x2{(_Float16)0, (_Float16)0}, one2 = f16x2{(_Float16)1, (_Float16)1};
                f16x2 up_c = hf(gup0);
                f16x2 h = zero2;
                f16x2 d_cur = hf(diag0) + hf(S[0]), d_prev = zero2;
                f16x2 bestf = hf(best);
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    f16x2 d_next = d_cur;
                    if (q + 1 < K) d_next = hf(Hl[q]) + hf(S[q + 1]);       // before Hl[q] is overwritten
                    h = __builtin_elementwise_maximum(__builtin_elementwise_maximum(d_cur, hf(El[q])), up_c);
                    Hl[q] = bits(h);
                    up_c = __builtin_elementwise_min(__builtin_elementwise_max(h + g_unit, zero2), one2);   // v_pk_add_f16 clamp
                    El[q] = bits(up_c);
                    if (q & 1) bestf = __builtin_elementwise_maximum(__builtin_elementwise_maximum(bestf, d_prev), d_cur);
                    else if (q == K - 1) bestf = __builtin_elementwise_maximum(bestf, d_cur);
                    d_prev = d_cur;
                    d_cur = d_next;
                }
                best = bits(bestf);
                h_last = bits(h);
                f_last = bits(up_c);
            } else if (LINF16) {
                // NW frame: h = max3(diag + S', left, up) -- perm, add, max3: three packed instructions per register
                auto hf = [](s16x2 v) __attribute__((always_inline)) { return __builtin_bit_cast(f16x2, v); };
                f16x2 h = hf(up0);
                f16x2 d_cur = hf(diag0) + hf(S[0]);
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    f16x2 d_next = d_cur;
                    if (q + 1 < K) d_next = hf(Hl[q]) + hf(S[q + 1]);       // before Hl[q] is overwritten
                    h = __builtin_elementwise_maximum(__builtin_elementwise_maximum(d_cur, hf(Hl[q])), h);
                    Hl[q] = __builtin_bit_cast(s16x2, h);
                    d_cur = d_next;
                }
                h_last = __builtin_bit_cast(s16x2, h);
            } else if (F16) {
                // Registers hold two half floats (bit patterns in the s16x2 containers).  pass1(q) -- diag + S
                // and E of row q, which only need the previous column -- is written between the links of the
                // dependent chain down the column (F, H, H - open), one row ahead.
                auto hf = [](s16x2 v) __attribute__((always_inline)) { return __builtin_bit_cast(f16x2, v); };
                auto bits = [](f16x2 v) __attribute__((always_inline)) { return __builtin_bit_cast(s16x2, v); };
                f16x2 d_cur, e_cur, d_prev = zero_half;
                auto pass1 = [&](int q, f16x2 &d, f16x2 &e) __attribute__((always_inline)) {
                    d = hf(q == 0 ? diag0 : Hl[q - 1]) + hf(S[q]);
                    const f16x2 e_open = F16SYM ? hf(HOl[q]) : hf(Hl[q]) + o_read_half;
                    e = __builtin_elementwise_maximum(TILT ? hf(El[q]) : hf(El[q]) + e_read_half, e_open);
                    if (ALG == kAlgSW) e = __builtin_elementwise_maximum(e, zero_half);     // folds into one max3: floors the cell
                    El[q] = bits(e);
                };
                f16x2 f = hf(fup0);
                f16x2 ho = hf(up0) + o_half;
                f16x2 h = zero_half;
                f16x2 bestf = hf(best);
                pass1(0, d_cur, e_cur);
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    f = __builtin_elementwise_maximum(TILT ? f : f + e_half, ho);
                    f16x2 d_next = zero_half, e_next = zero_half;
                    if (q + 1 < K) pass1(q + 1, d_next, e_next);        // before Hl[q] is overwritten
                    h = __builtin_elementwise_maximum(__builtin_elementwise_maximum(d_cur, e_cur), f);
                    Hl[q] = bits(h);
                    ho = h + o_half;
                    if (F16SYM) HOl[q] = bits(ho);
                    if (ALG == kAlgSW) {
                        if (q & 1) bestf = __builtin_elementwise_maximum(__builtin_elementwise_maximum(bestf, d_prev), d_cur);
                        else if (q == K - 1) bestf = __builtin_elementwise_maximum(bestf, d_cur);
                    }
                    d_prev = d_cur;
                    d_cur = d_next;
                    e_cur = e_next;
                }
                best = bits(bestf);
                h_last = bits(h);
                f_last = bits(f);
            } else if (SOURCES) {
                // Gap SOURCES instead of gap scores: El[q] holds XE, the best source of a horizontal gap in row q so
                // far (max over earlier columns k of H(q, k) - (j - 1 - k) ext), xf the same thing down the column (XF),
                // so E = XE - open and F = XF - open share one maximum and one subtract:
                //   g = max(XE, XF);  h = max(diag + S, g - open);  XE' = max(XE - ext, h);  XF' = max(XF - ext, h)
                // -- perm, add, 3 sub, 4 max: 9 packed instructions per register.  g is at least the cell to the left and
                // the cell above and never more than a cell that exists, so it feeds the running maximum as max(left, up)
                // does in the shared-gap kernel: kTrackNone / kTrackPair.  The chain xf -> g -> y -> h -> xf down the
                // column is strictly dependent; the next row's diag + S (which reads the OLD Hl[q]), the two extension
                // subtracts and the tracking are written between its links.
                s16x2 d_cur = diag0 + S[0];
                // XF of the lane above, 0 in the group's first lane.  Fetched here, behind the first add: at the head of
                // the step the DPP move follows the register's initialisation before the loop too closely, and the wait
                // state that costs lands inside the loop.
                s16x2 xf = as_pk(group_prev_or_zero<G>(as_u32(f_last), lmask)), h = pk(0);
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    const s16x2 g = pk_max(El[q], xf);
                    s16x2 d_next = pk(0);
                    if (q + 1 < K) d_next = Hl[q] + S[q + 1];
                    const s16x2 y = pk_sub_floor0(g, o_ref);
                    const s16x2 a = pk_sub_floor0(El[q], e_ref);
                    if (TRACK == kTrackAll) best = pk_max(best, d_cur);   // max = a diagonal arrival
                    if (TRACK == kTrackPair) best = pk_max(best, g);
                    h = pk_max(d_cur, y);
                    const s16x2 b = pk_sub_floor0(xf, e_ref);
                    Hl[q] = h;
                    El[q] = pk_max(a, h);
                    xf = pk_max(b, h);
                    d_cur = d_next;
                }
                if (TRACK == kTrackPair) best = pk_max(best, h);
                h_last = h;
                f_last = xf;
            } else if (SYM) {
                // h = max(diag + S, max(left, up) - g): one subtract for both gap directions.  The chain
                // max -> sub -> max down the column is strictly dependent; the next row's diag + S (which
                // reads the OLD left value just before it is overwritten) and the maximum tracking are
                // written between its links so that no two dependent packed instructions are adjacent.
                s16x2 h = up0;
                s16x2 d_cur = diag0 + S[0];
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    const s16x2 x = pk_max(Hl[q], h);
                    s16x2 d_next = pk(0);
                    if (q + 1 < K) d_next = Hl[q] + S[q + 1];
                    const s16x2 y = (ALG == kAlgSW) ? pk_sub_floor0(x, g_ref) : x;          // (NW frame: the gap step is free)
                    if (ALG == kAlgSW && TRACK == kTrackAll) best = pk_max(best, d_cur);   // max = a diagonal arrival
                    if (ALG == kAlgSW && TRACK == kTrackPair) best = pk_max(best, x);
                    h = pk_max(d_cur, y);
                    Hl[q] = h;
                    d_cur = d_next;
                }
                if (ALG == kAlgSW && TRACK == kTrackPair) best = pk_max(best, h);
                h_last = h;
            } else {
                // Everything of a row that only needs the previous column ("pass 1": diag + S, E, their
                // maximum, the SW maximum tracking) is computed one row ahead and written between the
                // links of the dependent chain down the column (F and H), so that no two dependent
                // packed instructions are adjacent.  pass1(q) reads the OLD Hl[q-1] / Hl[q] / HOl[q].
                auto pass1 = [&](int q) __attribute__((always_inline)) -> s16x2 {
                    const s16x2 d = (q == 0 ? diag0 : Hl[q - 1]) + S[q];
                    s16x2 e;
                    if (AFFSYM) {
                        e = pk_max((ALG == kAlgSW) ? pk_sub_floor0(El[q], e_read) : El[q], HOl[q]);
                        El[q] = e;
                    } else if (AFFINE) {
                        e = (ALG == kAlgSW)
                                ? pk_max(pk_sub_floor0(El[q], e_read), pk_sub_floor0(Hl[q], o_read))
                                : pk_max(El[q], pk_add_sat(Hl[q], o_read));
                        El[q] = e;
                    } else {
                        e = (ALG == kAlgSW) ? pk_sub_floor0(Hl[q], g_read) : Hl[q];
                    }
                    if (ALG == kAlgSW) best = pk_max(best, d);
                    return pk_max(d, e);
                };
                s16x2 h = up0, f = fup0;
                s16x2 ho = pk(0);
                if (AFFSYM) ho = (ALG == kAlgSW) ? pk_sub_floor0(up0, o_ref) : pk_add_sat(up0, o_ref);
                s16x2 m_cur = pass1(0);
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    if (AFFSYM) {
                        f = pk_max((ALG == kAlgSW) ? pk_sub_floor0(f, e_ref) : f, ho);
                    } else if (AFFINE) {
                        f = (ALG == kAlgSW) ? pk_max(pk_sub_floor0(f, e_ref), pk_sub_floor0(h, o_ref))
                                            : pk_max(f, pk_add_sat(h, o_ref));
                    } else {
                        f = (ALG == kAlgSW) ? pk_sub_floor0(h, g_ref) : h;
                    }
                    s16x2 m_next = pk(0);
                    if (q + 1 < K) m_next = pass1(q + 1);        // before Hl[q] is overwritten
                    h = pk_max(m_cur, f);
                    Hl[q] = h;
                    if (AFFSYM) {
                        ho = (ALG == kAlgSW) ? pk_sub_floor0(h, o_ref) : pk_add_sat(h, o_ref);
                        HOl[q] = ho;
                    }
                    m_cur = m_next;
                }
                h_last = h;
                f_last = f;
            }
            if (ALG == kAlgNW) {
                const s16x2 last = cell_sub(h_last, row_tilt);             // the last padded row's cell, out of the frame
                if (HALF) row_best = __builtin_bit_cast(s16x2, __builtin_elementwise_maximum(__builtin_bit_cast(f16x2, row_best),
                                                                                      __builtin_bit_cast(f16x2, last)));
                else row_best = pk_max(row_best, last);
            }
        }
        if (TILT) {
            top_row = cell_add(top_row, top_step);
            row_tilt = cell_add(row_tilt, col_step);
        }
        ++j;
        if constexpr (SOURCES) code_ptr += 2;
        else code_addr += 2;
    };

    using all_t = std::integral_constant<int, kTrackAll>;
    using first_t = std::integral_constant<int, ((SYM && ALG == kAlgSW) || SOURCES) ? kTrackNone : kTrackAll>;
    using second_t = std::integral_constant<int, ((SYM && ALG == kAlgSW) || SOURCES) ? kTrackPair : kTrackAll>;
    if constexpr (ALG == kAlgSW) {
        // Smith-Waterman needs no mask, from the first step to the last.  A lane left of column 0 reads zero-slab codes
        // (the pad), starts from all-zero registers and is handed zeros by the lane above, which is at the same column
        // one step earlier: its cells stay zero (half-float affine forms: its gap registers go negative, which the zero
        // floor of E hides exactly as at column 0).  A lane right of column F-1 reads zero-slab codes again -- padding
        // or N bases up to the batch's F, then the pad: every diag + S it offers the maximum is an H that exists
        // already, and it hands values only to lanes that are past the end as well.  So the whole sweep is ONE loop of
        // two-step trips and, where the step count is odd, one more step (a step rounded up instead would do as well,
        // but the compiler schedules the loop two VALU instructions per trip dearer without the step behind it).
        // Codes are read at most (last step) + 2 (prefetch) columns past F-1 and G-1 columns before column 0.
        static_assert(G - 1 + 1 + 2 <= kCodePad, "the unmasked sweep and its prefetch stay inside the code pad");
        const int steps = F + G - 1 - lead;
        int t = 0;
        bool biased = false;
        if constexpr (SOURCES) {
            biased = args.sym_max3_bias > 0;       // wave-uniform: the same sweep in its biased form
            // ... in the tilted frame (the bias: the low 16 bits); built for K <= 12 and for 8 x 19: the engine asks for it nowhere else
            const bool tilted = TILT_BUILT && biased && (args.sym_max3_bias >> 16) != 0;
            if constexpr (TILT_BUILT) if (tilted) {
                // THE TILTED BIASED FORM.  Cell (p, j) -- p the padded row, j the column -- is kept as value + B + x u with
                // u = p + j + c0 and x = -extend.  In that frame an extension costs nothing: E(p, j-1) - x IS the register of
                // (p, j-1) read in the frame of (p, j), F likewise down the column, the diagonal pays 2x through the profile
                // (S' = S + 2x, zero slab included), and ONE H - (o - x) serves E of the next column and F of the next row:
                //   d = diag + S';  e = max3(E, HO, floor);  f = max(f, ho);  h = max3(d, e, f);  ho = h - (o - x)
                // -- perm, add, 1 sub, 1 max, 2 max3: 6 packed instructions per register.  floor = B + x u is the zero of the
                // cell's own frame; as the third operand of E's max3 it floors the whole cell.
                // Lane l at step t holds row q of its K rows at u = l (K - 1) + q + t + 2 (c0 = 2 - lead), so within a lane
                // the floor depends on c = q + t alone: K floor registers, slot c % K, each read by one row per step and
                // moved K x on once row 0 has used it.  With the steady loop unrolled K steps deep every slot index is a
                // constant: the registers change names, nothing is copied.
                // THE WINDOW.  Every register starts, by formula, as the cell of an all-zero matrix, the smallest u (row -1
                // of the first lane before step 0) being 0.  e >= floor, h >= floor, ho >= floor - (o - x), f >= ho of the
                // row above, and d >= floor(p-1, j-1) + 2x - m = floor(p, j) - m: with B = 1024 + max(o - x, m)
                // (cell_rules.h: sym_affine_tilt_bias) no operand falls below 0x0400 -- but F above the group's first lane,
                // which is the zero of the lane shift: +0.0, it loses to every pattern of the window.  Every operand is a
                // value that exists in the matrix plus B + x u of the cell that reads it, u <= rows + F - lead, and the engine
                // launches this form only where that stays at or below 0x7BFF (sym_affine_tilt_ok).
                // A lane outside the columns or on padding rows fetches S' = 2x and stays exactly at its floors:
                // d = floor(p-1, j-1) + 2x = floor(p, j), e = max3(floor - x, floor - o, floor), f <= floor.
                // THE RUNNING MAXIMUM.  The diag + S' of one step carry K different tilts, those with the same c = q + t one:
                // an accumulator per live c in the floors' slots (how it is fed and carried: at the step below).
                // tests/test_sym_affine_tilted_sweep.py restates the frame on the CPU, tests/test_sym_affine_inframe_sweep.py
                // the sweep as it runs here.
                const int B = args.sym_max3_bias & 0xFFFF, xi = -(int)args.ext_ref;
                const int oxi = -(int)args.open_ref - xi;
                const s16x2 ox_c = pk((short)oxi), kx_c = pk((short)(K * xi));
                const int u0 = l * (K - 1);                                    // u of row -1 before step 0
                // THE HAND-OVER carries H - (o - x) of the lane's last row, which that lane has anyway (its ho): it is F's source
                // of row 0 as it comes, and row 0's diagonal one step later with the o - x back from the profile -- wave_setup
                // adds it to every score of a lane's row 0, zero slab included, for this loop only.  The moving border of the
                // group's first lane (row -1 as it reads it at step 0, one x on per step, zero below that lane) enters alike.
                s16x2 lead_border = as_pk(as_u32(pk((short)(B + xi - oxi))) & ~lmask);
                const s16x2 lead_step = as_pk(as_u32(pk((short)xi)) & ~lmask);
                // THE REMAINDER.  steps % K steps run first, as the LAST steps of a trip: the slots start out named as that
                // step finds them (row q of the first step reads slot (q + s0) % K) and nothing is copied to rotate them.
                // (Each step of that tail is conditional; where a skipped and a run step join the compiler places some register
                // copies.  Entering the trip through a switch, or leaving a trailing one through side exits, cost 146 and 495
                // VGPRs at 16 x 10 against 118: profiles/r20_sym_affine_inframe.txt.)
                const int s0 = K - steps % K;                                  // 1 .. K; K: no remainder
                s16x2 fl[K], acc[K], dprev[K];
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    Hl[q] = El[q] = pk((short)(B + xi * (u0 + q + 1)));
                    HOl[q] = Hl[q] - ox_c;
                    int c = q - s0;                                           // the anti-diagonal slot q stands for at step 0
                    c += c < 0 ? K : 0;
                    fl[q] = acc[q] = pk((short)(B + xi * (u0 + c + 2)));      // an accumulator at its floor holds 0
                    dprev[q] = Hl[q];                                         // (odd q) "row q at step -1": the floor of c = q - 1
                }
                up0 = pk((short)(B + xi * u0 - oxi));
                f_last = HOl[K - 1];
                // One step; row q reads slot (q + SLOT0) % K.  The pipelined fetches and the code pointer are the plain biased
                // step's.
                // THE RUNNING MAXIMUM STAYS IN THE FRAME.  Rows go in pairs: the d of an even row q and the previous step's d of
                // row q + 1 lie on the same anti-diagonal c = q + t and enter its accumulator in one max3, K / 2 per step.  When
                // row 0 completes its anti-diagonal the slot moves on to c + K, floor and accumulator alike (+ K x: the same value
                // read in the new frame), and the accumulator keeps collecting: it holds the largest cell so far plus B + x u of a
                // cell of the sweep, which sym_affine_tilt_ok bounds.  The K accumulators leave the frame once, after the last step.
                // THE CODE FETCHES are volatile: one LDS byte load each, waited for by the compiler as any other load.  In the
                // K-step trip their offsets are adjacent constants, and plain loads get merged into wide, unaligned ones whose
                // bytes come apart again on the VALU (18 instructions per trip at 16 x 10), which has no slot to spare; the LDS
                // port has.  profiles/r21_sym_affine_bookkeeping.txt.
                // THE ROW TABLES (FORM kRowTables; kLdsProfile is the step as described so far).  Where every S' fits a byte the lane
                // holds them -- Ta[q], Tb[q]: four bytes, row q against the four reference classes, pair A and pair B, built by
                // wave_setup_tables, EVERY row with o - x on top (S'' = S' + o - x) -- and a step fetches ONE selector dword
                // {ca, 0x0c, 4 + cb, 0x0c}: S''[q] = v_perm_b32(Tb[q], Ta[q], selector), the perm the profile's merge takes anyway.
                // No slab numbers, no address arithmetic, no profile loads; the stream is fetched two steps ahead (volatile, as the
                // code bytes are).
                // NO H REGISTERS.  Hl[q] is read only as the next step's diagonal of row q + 1, and HOl[q] = Hl[q] - (o - x) is kept
                // anyway (E's source).  So every row does what row 0 does with the handed-over ho: d[q] = HOl[q - 1] + S''[q], the
                // o - x back from the table.  (H + S') and (H - (o - x)) + (S' + (o - x)) are the same 16 bits; the byte rule counted
                // + (o - x) on every score already (sym_affine_row_table_high).  pass1(q + 1) reads HOl[q] before this step's ho
                // overwrites it, as it read Hl[q].  The row-table forms keep no Hl at all (28 VGPRs at 8 x 19); the LDS-profile form,
                // whose profile carries o - x in row 0 only, keeps it.
                // A base that is no ACGT, and every column of the pads, selects the constant 0x00 in its half: S'' = 0 where the
                // profile form adds 2x.  OUTSIDE A REFERENCE'S ACGT COLUMNS THAT IS EXACT, by one argument for every row:
                //   * left of column 0 every register holds its floor, HOl its floor less o - x (by induction from the start values).
                //     d = (floor(p-1, j-1) - (o - x)) + 0 = floor(p, j) - o - x: at or below the floor, so e = max3(floor - x,
                //     floor - o, floor) = floor wins h's max3, the accumulator's too, and the cell stays exactly at its floor as
                //     with S' = 2x.
                //   * right of a pair's last ACGT column (the wave sweeps on to its longest reference's) the profile form repeats
                //     cells that exist: S' = 2x makes d the cell (p-1, j-1) itself.  Every operation of the cell is monotone in its
                //     operands and d only got smaller (that cell less o + x), so by induction no register there exceeds what the
                //     profile form holds, the accumulators are offered nothing they have not seen, and the columns up to the last
                //     ACGT base -- which never read a column to their right -- are computed as before.
                //   * THE WINDOW.  Every cell that is computed has u >= 2 (u = l (K - 1) + q + t + 2): the smallest such d is
                //     B + 2x - o - x = B - (o - x) + x, at or above 0x0400 by the bias of the frame (B >= 1024 + o - x, x >= 0:
                //     sym_affine_tilt_bias, sym_affine_max3_ok); upwards nothing grew.  The rule has no scoring to refuse on the
                //     window's account.
                // A base that is no ACGT BEFORE its reference's last ACGT base must score exactly 2x, which a table cannot give:
                // wave_setup_tables finds such a wave (`repair`, wave-uniform) and it runs FORM kRowTablesRepair, the same step with
                // every half that selected 0x00 set to 2x + o - x (zero_0: a non-negative byte by the same rule, OR-ed onto a half
                // that is 0) -- one v_or_b32 per register and four per step more: the profile's scores at every column, pads
                // included, so exact by the profile form's argument.
                // WORD ARITHMETIC (both row-table forms; the LDS-profile form keeps its packed instructions: its S' may be negative
                // and its o - x is not bounded below by a rule).  The adds and the subtract of the step are 32-bit ones on the packed
                // word -- v_add_u32 / v_sub_u32 issue in the full-rate class, v_pk_add_u16 / v_pk_sub_i16 in the half-rate one
                // (profiles/r02_valu_rate_bitops.txt) -- which is the packed result bit for bit because no half carries or borrows
                // into its neighbour.  Per operand, smallest and largest half:
                //   d = diag + S''     diag in [0x0400, 0x7BFF]: an HO of the window (above) or the border; S'' in [0, 255]
                //                      (sym_affine_row_tables_ok: every table byte and zero_0); the sum is an operand of h's max3,
                //                      at most 0x7BFF (sym_affine_tilt_ok).  No carry.
                //   ho = h - (o - x)   h in [floor, 0x7BFF], floor >= B >= 0x0400 + (o - x), o - x in [0, 255]
                //                      (sym_affine_row_tables_ok, sym_affine_tilt_bias): ho >= 0x0400.  No borrow.
                //   acc, fl + K x      acc, fl in [0x0400, 0x7BFF]; K x <= x * top index <= 0x77FF (sym_affine_tilt_ok: rows >= K):
                //                      the sum stays below 0x10000.  (It is within 0x7BFF wherever a maximum reads it afterwards;
                //                      the last move of a slot may lie past the top index, read by the closing subtract alone.)
                //   lead_border + lead_step   the group's first lane: B + x - (o - x) + x t in [0x0400, 0x7BFF], x >= 0; every
                //                      other lane: both halves 0 + 0, the masked halves stay 0.
                // tests/test_sym_affine_word_arith.py asserts these bounds operand by operand and the equality of every register,
                // word against halves.
                // tests/test_sym_affine_row_tables_sweep.py restates the step on the CPU with the H registers it had.
                // 8 x 19 (TABLES_ONLY).  K is odd: rows 0 .. 17 enter the accumulators in pairs as above, and row 18, which has no
                // partner, enters the slot of its own anti-diagonal c = 18 + t alone, at once, with ONE two-operand packed maximum.
                // That keeps the running maximum exact by the same anti-diagonal argument with one operand fewer: every d of
                // anti-diagonal c still reaches slot c before row 0 completes c and the slot moves on (row 18 at step c - 18, the
                // pairs as before, row 1 with row 0 at step c), each d enters exactly one slot, and a two-operand half-float
                // maximum of two patterns of the window is the integer maximum as the three-operand one is.  After the last step
                // only odd rows wait in dprev, as for an even K.  Its stream is the compact one (wave_setup_tables): one volatile
                // 16-bit LDS load two steps ahead, widened to the selector dword by one v_perm_b32 when its step comes.
                // tests/test_sym_affine_odd_tile_sweep.py restates this step on the CPU.
                constexpr int kLdsProfile = 0, kRowTables = 1, kRowTablesRepair = 2;
                constexpr bool SEL16 = TABLES_ONLY;
                typedef __attribute__((address_space(3))) const unsigned short lds_cu16;
                lds_cu32 *sel_ptr = (lds_cu32 *)(lds_offset(w.refc) + grp * args.refc_stride - 4 * (l - lead));   // + 4 per step
                lds_cu16 *sel16_ptr = (lds_cu16 *)(lds_offset(w.refc) + grp * args.refc_stride - 2 * (l - lead));  // (compact: + 2 per step)
                unsigned sel_cur = 0, sel_next = 0;
                if constexpr (SEL16) {
                    sel_cur = __builtin_amdgcn_perm(kSelZero4, (unsigned)sel16_ptr[0], kSelWiden);
                    sel_next = sel16_ptr[1];                              // (kept narrow until its step)
                } else if (tables) {
                    sel_cur = sel_ptr[0];
                    sel_next = sel_ptr[1];
                }
                const unsigned zero_0 = as_u32(pk((short)(s_zero + s_row0)));
                auto tilted_step = [&](auto slot_tag, auto form_tag) __attribute__((always_inline)) {
                    constexpr int SLOT0 = decltype(slot_tag)::value;
                    constexpr int FORM = decltype(form_tag)::value;
                    // the step's adds and its subtract: on the 32-bit word in the row-table forms (WORD ARITHMETIC, above)
                    auto add2 = [](s16x2 a, s16x2 b) __attribute__((always_inline)) {
                        if constexpr (FORM != kLdsProfile) return as_pk(as_u32(a) + as_u32(b));
                        else return a + b;
                    };
                    auto sub2 = [](s16x2 a, s16x2 b) __attribute__((always_inline)) {
                        if constexpr (FORM != kLdsProfile) return as_pk(as_u32(a) - as_u32(b));
                        else return a - b;
                    };
                    s16x2 S[K], d[K];
                    const s16x2 diag0 = up0;
                    if constexpr (lmap::kInterleaved) up0 = row_prev_or<lmap::kStride>(HOl[K - 1], lead_border);
                    else up0 = group_prev_or<G>(HOl[K - 1], lead_border, lmask);
                    lead_border = add2(lead_border, lead_step);
                    if constexpr (FORM == kLdsProfile) {
                        merge_profile<K>(pa, pb, S);
                        lds_load_lane<K>(lane_base + ca_next * geo::kPairStride, pa);
                        lds_load_lane<K>(lane_base + cb_next * geo::kPairStride, pb);
                        ca_next = ((volatile lds_cu8 *)code_ptr)[4];
                        cb_next = ((volatile lds_cu8 *)code_ptr)[5];
                    } else {
#pragma unroll
                        for (int q = 0; q < K; ++q) S[q] = as_pk(__builtin_amdgcn_perm(Tb[q], Ta[q], sel_cur));
                        if constexpr (FORM == kRowTablesRepair) {
                            // bit 3 of a selector byte is set where it is 0x0c: 0xFFFF in the halves that selected the constant
                            const unsigned none = ((sel_cur >> 3) & 0x00010001u) * 0xFFFFu;
                            const unsigned fix_0 = zero_0 & none;           // (a non-negative byte per half, as every table byte is)
#pragma unroll
                            for (int q = 0; q < K; ++q) S[q] = as_pk(as_u32(S[q]) | fix_0);
                        }
                        if constexpr (SEL16) {
                            sel_cur = __builtin_amdgcn_perm(kSelZero4, sel_next, kSelWiden);
                            sel_next = ((volatile lds_cu16 *)sel16_ptr)[2];
                            sel16_ptr += 1;
                        } else {
                            sel_cur = sel_next;
                            sel_next = ((volatile lds_cu32 *)sel_ptr)[2];
                            sel_ptr += 1;
                        }
                    }
                    s16x2 e_cur;
                    auto pass1 = [&](int q, s16x2 &e) __attribute__((always_inline)) {
                        if constexpr (FORM == kLdsProfile) d[q] = add2(q == 0 ? diag0 : Hl[q - 1], S[q]);
                        else d[q] = add2(q == 0 ? diag0 : HOl[q - 1], S[q]);     // (NO H REGISTERS: o - x rides on every row's table)
                        e = pk_max3_h(El[q], HOl[q], fl[(q + SLOT0) % K]);
                        El[q] = e;
                    };
                    s16x2 ho = up0;
                    pass1(0, e_cur);
                    // F of the lane above, the shift's zero in the group's first lane (fetched behind the first row's pass 1)
                    s16x2 f = pk(0), h = pk(0);
                    if constexpr (lmap::kInterleaved) f = as_pk(row_prev_or_zero<lmap::kStride>(as_u32(f_last)));
                    else f = as_pk(group_prev_or_zero<G>(as_u32(f_last), lmask));
#pragma unroll
                    for (int q = 0; q < K; ++q) {
                        f = pk_max_h(f, ho);
                        s16x2 e_next = pk(0);
                        if (q + 1 < K) pass1(q + 1, e_next);            // before Hl[q] / HOl[q] is overwritten
                        h = pk_max3_h(d[q], e_cur, f);
                        if constexpr (FORM == kLdsProfile) Hl[q] = h;
                        ho = sub2(h, ox_c);
                        HOl[q] = ho;
                        if (!(q & 1)) {
                            s16x2 &a = acc[(q + SLOT0) % K];
                            if (q + 1 < K) a = pk_max3_h(a, d[q], dprev[q + 1]);
                            else a = pk_max_h(a, d[q]);                  // (odd K: the unpaired last row)
                        }
                        e_cur = e_next;
                    }
#pragma unroll
                    for (int q = 1; q < K; q += 2) dprev[q] = d[q];
                    f_last = f;
                    // row 0's anti-diagonal is complete: the slot moves on to c + K
                    acc[SLOT0 % K] = add2(acc[SLOT0 % K], kx_c);
                    fl[SLOT0 % K] = add2(fl[SLOT0 % K], kx_c);
                    if constexpr (FORM == kLdsProfile) code_ptr += 2;
                };
                auto tilted_sweep = [&](auto form_tag) __attribute__((always_inline)) {
                    unrolled_steps(std::make_integer_sequence<int, K>{}, [&](auto slot_tag) __attribute__((always_inline)) {
                        if constexpr (decltype(slot_tag)::value > 0) {
                            if (decltype(slot_tag)::value >= s0) tilted_step(slot_tag, form_tag);
                        }
                    });
                    for (int trips = steps / K; trips > 0; --trips)
                        unrolled_steps(std::make_integer_sequence<int, K>{}, [&](auto slot_tag) __attribute__((always_inline)) { tilted_step(slot_tag, form_tag); });
                };
                // One copy of the tail and the trip per form, each under a comparison of its own: written as if / else the copies'
                // common parts get hoisted and the kernel allocates half as many registers again
                // (profiles/r21_sym_affine_bookkeeping.txt, section 1).
                int form = __builtin_amdgcn_readfirstlane(tables ? (repair ? kRowTablesRepair : kRowTables) : kLdsProfile);
                if constexpr (!TABLES_ONLY) if (form == kLdsProfile) tilted_sweep(std::integral_constant<int, kLdsProfile>{});
                asm volatile("" : "+s"(form));          // (each comparison on a value the compiler knows nothing about)
                if (form == kRowTables) tilted_sweep(std::integral_constant<int, kRowTables>{});
                asm volatile("" : "+s"(form));
                if (form == kRowTablesRepair) tilted_sweep(std::integral_constant<int, kRowTablesRepair>{});
                // the odd rows of the last step, then out of the frame: after a whole trip slot q stands for c = q + steps
                best = pk(0);
#pragma unroll
                for (int q = 0; q + 1 < K; q += 2) acc[q] = pk_max_h(acc[q], dprev[q + 1]);
#pragma unroll
                for (int q = 0; q < K; ++q) best = pk_max(best, acc[q] - fl[q]);
            }
            if constexpr (!TABLES_ONLY) if (biased && !tilted) {
                const s16x2 bias_c = pk((short)args.sym_max3_bias);
                const s16x2 lead_bias = as_pk(as_u32(bias_c) & ~lmask);          // the bias in the group's first lane, zero below it
                // One step of the biased form.  The hand-over, the pipelined fetches and the code pointer are the step's above.
                auto biased_step = [&](s16x2 (&S)[K]) __attribute__((always_inline)) {
                    const s16x2 diag0 = up0;
                    up0 = group_prev_or<G>(h_last, lead_bias, lmask);      // the group's first lane reads the bias, the zero of this form
                    merge_profile<K>(pa, pb, S);
                    lds_load_lane<K>(lane_base + ca_next * geo::kPairStride, pa);
                    lds_load_lane<K>(lane_base + cb_next * geo::kPairStride, pb);
                    ca_next = code_ptr[4];
                    cb_next = code_ptr[5];
                    // Every cell is kept as value + B (bias_c) and the Gotoh cell of the half-float kernel above runs on it: adds
                    // and subtracts are plain packed int16, maxima go three at a time through v_pk_maximum3_f16 --
                    //   d = diag + S;  e = max3(E - ext, HO, B);  f = max(f - ext, ho);  h = max3(d, e, f);  ho = h - open
                    // -- perm, add, 3 sub, 1 max, 2 max3: 8 packed instructions per register, plus K / 2 for the tracking (every
                    // step: gap scores, not sources, so there is no pair trick).  B in E's max3 is the zero floor of the whole cell.
                    // THE WINDOW.  A half-float maximum is an integer maximum as long as every operand's bit pattern lies in
                    // [0x0400, 0x7BFF].  With o = -open, x = -ext, m = max(0, -mismatch, -match):  e >= B,  h >= B,  ho >= B - o,
                    // f >= ho >= B - o (by induction from the border f = B),  e - ext >= B - x,  f - ext >= B - o - x,  d >= B - m,
                    // so B = 1024 + o + x + m (sym_affine_bias) keeps every operand at or above 0x0400 and no subtract wraps or needs
                    // a clamp; nothing exceeds B + the largest cell, and the engine launches this form only where that is at most
                    // 0x7BFF (sym_affine_max3_ok).  Nothing is ever converted to or from a half float.  A lane outside the columns
                    // or on padding rows fetches scores of 0 and stays at exactly B: max3(B, max3(B - x, B - o, B), max(B - x, B - o)).
                    // pass1(q) -- diag + S and E of row q, which only need the previous column -- sits between the links of the
                    // dependent chain down the column (f, h, ho), one row ahead, as in the half-float kernel.
                    s16x2 d_cur, e_cur, d_prev = bias_c;
                    auto pass1 = [&](int q, s16x2 &d, s16x2 &e) __attribute__((always_inline)) {
                        d = (q == 0 ? diag0 : Hl[q - 1]) + S[q];
                        e = pk_max3_h(El[q] - e_read, HOl[q], bias_c);
                        El[q] = e;
                    };
                    s16x2 ho = up0 - o_ref;
                    pass1(0, d_cur, e_cur);
                    // F of the lane above, B in the group's first lane (fetched behind the first row's pass 1: see the gap-source form)
                    s16x2 f = group_prev_or<G>(f_last, lead_bias, lmask), h = bias_c;
#pragma unroll
                    for (int q = 0; q < K; ++q) {
                        f = pk_max_h(f - e_ref, ho);
                        s16x2 d_next = bias_c, e_next = bias_c;
                        if (q + 1 < K) pass1(q + 1, d_next, e_next);        // before Hl[q] is overwritten
                        h = pk_max3_h(d_cur, e_cur, f);
                        Hl[q] = h;
                        ho = h - o_ref;
                        HOl[q] = ho;
                        if (q & 1) best = pk_max3_h(best, d_prev, d_cur);
                        else if (q == K - 1) best = pk_max_h(best, d_cur);
                        d_prev = d_cur;
                        d_cur = d_next;
                        e_cur = e_next;
                    }
                    h_last = h;
                    f_last = f;
                    code_ptr += 2;
                };
                // every border is B, H - open of the border B - open
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    Hl[q] = El[q] = bias_c;
                    HOl[q] = bias_c - o_ref;
                }
                up0 = h_last = f_last = best = bias_c;
                for (; t + 1 < steps; t += 2) {        // (gap scores, not sources: both steps of a trip track)
                    biased_step(S0);
                    biased_step(S1);
                }
                if (t < steps) biased_step(S0);
                best = best - bias_c;                  // the score is best - B
            }
        }
        if constexpr (!TABLES_ONLY) if (!biased) {
            for (; t + 1 < steps; t += 2) {        // two steps per trip: loop-carried registers swap roles
                step(std::false_type{}, first_t{}, S0, S1);    // instead of being copied (+4 % SW, +4 % affine
                step(std::false_type{}, second_t{}, S1, S0);   // together with the pipelined fetch)
            }
            if (t < steps) step(std::false_type{}, all_t{}, S0, S1);
        }
    } else {
        // The NW variant's result needs every lane frozen at the last column: its fill and drain steps stay masked
        const int steps = F + G - 1;
        const int fill_end = G - 1 < steps ? G - 1 : steps;
        const int steady_end = F > fill_end ? F : fill_end;
        int t = 0;
        auto single = [&](auto masked_tag) __attribute__((always_inline)) { step(masked_tag, all_t{}, S0, S1); };
        for (; t < fill_end; ++t) single(std::true_type{});
        {                                          // two steps per trip (+10 % NW linear)
            for (; t + 1 < steady_end; t += 2) {
                step(std::false_type{}, first_t{}, S0, S1);
                step(std::false_type{}, second_t{}, S1, S0);
            }
        }
        for (; t < steady_end; ++t) single(std::false_type{});
        for (; t < steps; ++t) single(std::true_type{});
    }

    // ---- result ----
    s16x2 res;
    if (LINF16_SW) {
        const f16x2 b = __builtin_bit_cast(f16x2, best);
        res = s16x2{(short)(int)((float)b.x * 1024.0f), (short)(int)((float)b.y * 1024.0f)};
    } else if (HALF) {
        f16x2 b = __builtin_bit_cast(f16x2, best);
        if (ALG == kAlgNW) {          // max(0, last column of every row, last row of every column), out of the tilt
            b = __builtin_bit_cast(f16x2, l == G - 1 ? row_best : cell(-rcentre));
#pragma unroll
            for (int q = 0; q < K; ++q)
                b = __builtin_elementwise_maximum(b, __builtin_bit_cast(f16x2, cell_sub(Hl[q], cell(tilt_row * (l * K + q) + tilt_col * F - centre + rcentre))));
            // b >= -rcentre (the zero of the result rule); the rest of the score comes back as an integer
            res = s16x2{(short)((int)b.x + rcentre), (short)((int)b.y + rcentre)};
        } else {
            res = s16x2{(short)(int)b.x, (short)(int)b.y};
        }
    } else if (ALG == kAlgSW) {
        res = best;
    } else {
        // last column: every lane froze at column F-1; last row: last register of lane G-1
        s16x2 col = l == G - 1 ? row_best : pk(0);
#pragma unroll
        for (int q = 0; q < K; ++q) col = pk_max(col, Hl[q] - cell(tilt_row * (l * K + q) + tilt_col * F));
        res = pk_max(col, pk(0));
    }
#pragma unroll
    for (int i = 0; i < lmap::kReduceSteps; ++i)             // over the lanes of the group: G / 2 ... 1 lanes apart, times the map's stride
        res = pk_max(res, as_pk((unsigned)__shfl_xor((int)as_u32(res), lmap::reduce_distance(i), kWave)));
    if (l == 0) {
        const long long pa = pair0 + 2 * grp;
        if (pa + 1 < n_pairs && ((unsigned long long)scores & 3ull) == 0) {
            *reinterpret_cast<unsigned *>(scores + pa) = as_u32(res);
        } else {
            if (pa < n_pairs) scores[pa] = res.x;
            if (pa + 1 < n_pairs) scores[pa + 1] = res.y;
        }
    }
}

// ---- host-side geometry: LDS bytes one wave needs for shape (R, F) ----
struct WaveLds {
    int prof_area, refc_stride, total;
};

template <int G, int K>
inline WaveLds wave_lds(int R, int F) {
    using geo = Geo<G, K>;
    WaveLds w;
    const int raw_refs = ((2 * F + 16 + 15) / 16) * 16;              // one lane group's two references, staged raw, then overwritten
    w.prof_area = geo::kProfBytes > raw_refs ? geo::kProfBytes : raw_refs;
    w.prof_area = ((w.prof_area + 15) / 16) * 16;
    w.refc_stride = ((2 * (F + 2 * kCodePad) + 15) / 16) * 16;
    w.total = w.prof_area + geo::kGroups * w.refc_stride + ((geo::kPairs * 8 + 15) / 16) * 16;
    return w;
}

// ... and with the row tables (wave_setup_tables): prof_area holds the wave's raw references, refc_stride is one group's selector
// stream, and the raw reads are staged where the streams are built afterwards.  A group's lanes read G consecutive dwords of
// its stream: a stride of G (mod 64) dwords puts the groups of a wave on disjoint banks.
inline WaveLds row_table_lds(int G, int R, int F) {
    const int groups = kWave / G, pairs = 2 * groups;
    WaveLds w;
    w.prof_area = ((pairs * F + 32 + 15) / 16) * 16;
    int stride_dw = F + 2 * row_table_pad(G);
    stride_dw += ((G - stride_dw) % 64 + 64) % 64;
    w.refc_stride = 4 * stride_dw;
    const int streams = groups * w.refc_stride, raw_reads = ((pairs * R + 32 + 15) / 16) * 16;
    w.total = w.prof_area + (streams > raw_reads ? streams : raw_reads);
    return w;
}

// ... and with the compact stream of the 8 x 19 tile: 16 bits per column and group.  The 8 lanes of a group read 8 consecutive
// entries, 16 bytes that touch up to five dwords wherever they start; ds_read_u16 is served 32 lanes -- four groups -- at a time on
// banks (a / 4) mod 32, so a group stride of 8 (mod 64) dwords, the dword stream's `G mod 64`, keeps the four windows of a
// half-wave on disjoint banks (two lanes in one dword read the same address: a broadcast).  150 x 500: 8,032 B of raw references +
// 8 x 1,056 B of streams = 16,480 B per wave, 65,920 B per 4-wave block (the dword stream: 26,720 and 106,880).
// (the arithmetic is cell_constants.h's, where the rule that budgets it reads it too)
static_assert(kSideTilePad == row_table_pad(kSideTileG) && kSideTilePairs == 2 * (kWave / kSideTileG), "cell_constants.h restates the side tile's layout");
inline WaveLds row_table_lds16(int R, int F) {
    WaveLds w;
    w.prof_area = side_tile_refs_area(F);
    w.refc_stride = side_tile_stream_stride(F);
    w.total = side_tile_wave_lds(R, F);
    return w;
}

}  // namespace valign
