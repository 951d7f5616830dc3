// engine.hip.h -- the host side of libHIPKernel.so: one Engine per (device, read_length, ref_length, scoring).
//
// The class is declared here; its parts are separate translation units, compiled in parallel and testable apart:
//   engine_core.hip ..... construction, launch-plan selection (cost model), staging, describe()
//   cell_rules.h ........ the cell-range rules and the choice of gap form, fill kernel and alignment path (pure, CPU-tested)
//   engine_score.hip .... score_alignments: register-sweep launches, the host-pointer chunk pipeline, 4-bit class
//                         unpacking, length-sorted batches (reference: DefaultKernel.cpp:52-202).  The pipeline's pieces are
//                         defined here once -- host_chunk_pairs, stage_chunk, wait_slot -- and so is record_pipeline, the
//                         whole pipeline of the calls that bring fixed-size records back (placed and spanned scores)
//   engine_long.hip ..... long reads: row strips (score_long_kernel) and the banded block chain (score_band_kernel)
//   long_plan.h ......... the route of a long-read score call, its compiled instances, strip sizes and the chain's plan (pure, CPU-tested)
//   engine_align.hip .... compute_alignments: fill + traceback launches, row strips, the fused small-batch launch, the
//                         host-pointer pipeline with its copy-issuing thread (reference: DefaultKernel.cpp:21-50, 204-525)
//   engine_placed.hip ... placed Smith-Waterman scores: score + end cell from the score sweep (placed_kernels.hip.h); owns
//                         score_placed_strips, the ONE pointer-free strip sweep (int16 strips and the int32 sweep are two
//                         PlacedSweep descriptions of it); its host call is record_pipeline with a one-line launch
//   engine_span.hip ..... spanned Smith-Waterman scores: a placed score plus the begin cell, from a second placed sweep over the
//                         reversed prefixes (span_kernels.hip.h); its host call is record_pipeline too
//   engine_subopt.hip ... suboptimal Smith-Waterman scores: the placed sweep's suboptimal form, which also leaves the column
//                         maxima in a scratch, and subopt_records_kernel (subopt_kernels.hip.h); record_pipeline again
//   engine_extend.hip ... extension scores: the anchored score, its end cell and the read-end score from one sweep with gap-priced
//                         borders and no floor (extend_kernels.hip.h) or, under extend_wide = 1, from score_placed_strips with the
//                         int32 extension sweep (extend_wide_kernels.hip.h); record_pipeline again
//   engine_cigar.hip .... the compact result format: records + CIGAR ops encoded on the device behind the walks (cigar_kernels.hip.h)
//   engine_span_cigar.hip spanned CIGARs: the alignment of the span from the span's window -- the forward placed sweep, the
//                         reversal, the child engine's ALIGNMENT of the reversed prefixes and the backward encoder
//                         (span_cigar_kernels.hip.h) behind its walk
//   engine_extend_align.hip  extension alignments: the extension sweep with back pointers, the walk from the chosen end cell to
//                         the anchor, the compact result format's encoder (extend_align_kernels.hip.h)
//   hip_plugin.hip ...... the plugin ABI and the flat C API over it
// The closest reference precedent for the staging loops is the OpenCL backend's gather / copy / launch / collect loop
// (src/Kernels/OpenCL/OpenCLKernel.cpp:57-108); unlike it, chunks here are large, asynchronous and overlapped.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "align_parts.h"
#include "cell_rules.h"
#include "extend_zdrop.h"
#include "hip_handles.h"
#include "host_pipeline.h"
#include "kernel_instances.hip.h"
#include "band_kernels.hip.h"
#include "cigar_kernels.hip.h"
#include "long_kernels.hip.h"
#include "long_plan.h"
#include "pack_kernels.hip.h"
#include "ragged_kernels.hip.h"
#include "span_kernels.hip.h"
#include "span_cigar_kernels.hip.h"
#include "subopt_kernels.hip.h"
#include "strip_kernels.hip.h"
#include "strip_plan.h"

namespace valign {

// The per-geometry kernels are compiled in kernel_part.hip (one object per part, in parallel)
#define VALIGN_DECLARE_FULL(G, K) VALIGN_FAST_KERNELS(extern template, G, K) VALIGN_FALLBACK_KERNELS(extern template, G, K)
#define VALIGN_DECLARE_FAST(G, K) VALIGN_FAST_KERNELS(extern template, G, K)
VALIGN_ALL_PARTS(VALIGN_DECLARE_FULL, VALIGN_DECLARE_FAST)
#undef VALIGN_DECLARE_FULL
#undef VALIGN_DECLARE_FAST
VALIGN_SIDE_KERNELS(extern template)

// One compiled (G, K) geometry with its kernel variants.
struct Geometry {
    int G, K;
    bool full;                     // carries the fallback kernels too (kernel_instances.hip.h)
    WaveLds (*lds)(int R, int F);
    const void *kernel[2][7];      // score kernels [alg][linear, symmetric linear, affine, symmetric affine,
                                   //                     symmetric affine / affine / symmetric linear on half floats]
    const void *fill[2][kFillKernels];      // alignment fill kernels [alg][FillKernel]; nullptr: not compiled for this geometry
    const void *(*placed)(int track, int gaps);      // placed-score kernels (placed_kernels.hip.h); returns nullptr where none is compiled
    const void *(*subopt)(int track, int gaps);      // suboptimal-score kernels: the full geometries', nullptr elsewhere
    const void *(*extend)(int gaps);                 // extension-score kernels (extend_kernels.hip.h): the full geometries', nullptr elsewhere
    const void *(*extend_align)(int affine);         // extension-alignment fills (extend_align_kernels.hip.h): the full geometries', nullptr elsewhere
    const void *(*extend_zdrop)(int gaps);           // ... and the ZDROP forms of both (key extend_zdrop_rows): wherever the plain form exists
    const void *(*extend_align_zdrop)(int affine);
};

template <int G, int K>
constexpr void set_fast_kernels(Geometry &g) {
    g.kernel[0][0] = (const void *)&score_kernel<G, K, kAlgSW, kGapLinear>;
    g.kernel[0][1] = (const void *)&score_kernel<G, K, kAlgSW, kGapSym>;
    g.kernel[0][2] = (const void *)&score_kernel<G, K, kAlgSW, kGapAffine>;
    g.kernel[0][3] = (const void *)&score_kernel<G, K, kAlgSW, kGapAffineSym>;
    g.kernel[0][4] = (const void *)&score_kernel<G, K, kAlgSW, kGapAffineSymF16>;
    g.kernel[0][5] = (const void *)&score_kernel<G, K, kAlgSW, kGapAffineF16>;
    g.kernel[0][6] = (const void *)&score_kernel<G, K, kAlgSW, kGapSymF16>;
    g.kernel[1][0] = (const void *)&score_kernel<G, K, kAlgNW, kGapLinear>;
    g.kernel[1][1] = (const void *)&score_kernel<G, K, kAlgNW, kGapSym>;
    g.kernel[1][2] = (const void *)&score_kernel<G, K, kAlgNW, kGapAffine>;
    g.kernel[1][3] = (const void *)&score_kernel<G, K, kAlgNW, kGapAffineSym>;
    g.kernel[1][4] = (const void *)&score_kernel<G, K, kAlgNW, kGapAffineSymF16>;
    g.kernel[1][5] = (const void *)&score_kernel<G, K, kAlgNW, kGapAffineF16>;
    g.kernel[1][6] = (const void *)&score_kernel<G, K, kAlgNW, kGapSymF16>;
    g.fill[0][kFillTagKey] = (const void *)&align_fill_tag_kernel<G, K, kAlgSW, true, false>;
    g.fill[0][kFillTagProfKey] = (const void *)&align_fill_tag_kernel<G, K, kAlgSW, true, false, false, true>;
    g.fill[0][kFillAffineTagSym] = (const void *)&align_fill_affine_tag_kernel<G, K, kAlgSW, true>;
    g.fill[1][kFillTag] = (const void *)&align_fill_tag_kernel<G, K, kAlgNW, false, false>;
    g.fill[1][kFillAffineTagSym] = (const void *)&align_fill_affine_tag_kernel<G, K, kAlgNW, true>;
}

template <int G, int K>
constexpr Geometry fast_geometry() {
    Geometry g{G, K, false, &wave_lds<G, K>, {}, {}, &placed_kernel<G, K, false>, &subopt_kernel<G, K, false>, &extend_kernel<G, K, false>, &extend_align_kernel<G, K, false>,
               &extend_zdrop_kernel<G, K, false>, &extend_align_zdrop_kernel<G, K, false>};
    set_fast_kernels<G, K>(g);
    return g;
}

template <int G, int K>
constexpr Geometry full_geometry() {
    Geometry g{G, K, true, &wave_lds<G, K>, {}, {}, &placed_kernel<G, K, true>, &subopt_kernel<G, K, true>, &extend_kernel<G, K, true>, &extend_align_kernel<G, K, true>,
               &extend_zdrop_kernel<G, K, true>, &extend_align_zdrop_kernel<G, K, true>};
    set_fast_kernels<G, K>(g);
    g.fill[0][kFillLinear] = (const void *)&align_fill_kernel<G, K, kAlgSW, false>;
    g.fill[0][kFillLinearSym] = (const void *)&align_fill_kernel<G, K, kAlgSW, true>;
    g.fill[0][kFillAffine] = (const void *)&align_fill_affine_kernel<G, K, kAlgSW, false>;
    g.fill[0][kFillAffineSym] = (const void *)&align_fill_affine_kernel<G, K, kAlgSW, true>;
    g.fill[0][kFillSse] = (const void *)&align_fill_sse_kernel<G, K, kAlgSW>;
    g.fill[0][kFillTag] = (const void *)&align_fill_tag_kernel<G, K, kAlgSW, false, false>;
    g.fill[0][kFillSseTag] = (const void *)&align_fill_tag_kernel<G, K, kAlgSW, false, true>;
    g.fill[1][kFillLinear] = (const void *)&align_fill_kernel<G, K, kAlgNW, false>;
    g.fill[1][kFillLinearSym] = (const void *)&align_fill_kernel<G, K, kAlgNW, true>;
    g.fill[1][kFillAffine] = (const void *)&align_fill_affine_kernel<G, K, kAlgNW, false>;
    g.fill[1][kFillAffineSym] = (const void *)&align_fill_affine_kernel<G, K, kAlgNW, true>;
    g.fill[1][kFillSse] = (const void *)&align_fill_sse_kernel<G, K, kAlgNW>;
    g.fill[0][kFillSseTagKey] = (const void *)&align_fill_tag_kernel<G, K, kAlgSW, true, true>;
    g.fill[0][kFillAffineTag] = (const void *)&align_fill_affine_tag_kernel<G, K, kAlgSW, false>;
    g.fill[1][kFillSseTag] = (const void *)&align_fill_tag_kernel<G, K, kAlgNW, false, true>;
    g.fill[1][kFillAffineTag] = (const void *)&align_fill_affine_tag_kernel<G, K, kAlgNW, false>;
    return g;
}

// Rows covered = G*K.  Ordered by capacity; selection is by estimated cost (Engine::choose_plan).  The full geometries --
// one per row capacity 64 / 160 / 320 / 512 / 1024 / 2048 -- are where calls that need a fallback kernel are re-planned to.
static const Geometry kGeometries[] = {
    fast_geometry<8, 4>(),   fast_geometry<8, 6>(),   full_geometry<8, 8>(),   fast_geometry<16, 4>(),
    fast_geometry<8, 10>(),  fast_geometry<8, 12>(),  fast_geometry<16, 8>(),  full_geometry<16, 10>(),
    fast_geometry<16, 12>(), fast_geometry<32, 8>(),  full_geometry<32, 10>(), fast_geometry<32, 12>(),
    full_geometry<64, 8>(),  fast_geometry<64, 12>(), full_geometry<64, 16>(), fast_geometry<64, 24>(),
    full_geometry<64, 32>(),
};
constexpr int kNumGeometries = sizeof(kGeometries) / sizeof(kGeometries[0]);
#define VALIGN_COUNT(G, K) +1
static_assert(kNumGeometries == 0 VALIGN_ALL_PARTS(VALIGN_COUNT, VALIGN_COUNT), "kernel_instances.hip.h lists other geometries than this table");
#undef VALIGN_COUNT

// The side geometry (kernel_instances.hip.h): 8 x 19 with ONE kernel, [SW][symmetric affine], and the compact row-table stream's
// LDS.  It is in no table: only Engine::score_plan_for hands it out, where sym_affine_side_tile_refusal (cell_rules.h) is empty.
// ONE object, defined in engine_core.hip.
extern const Geometry kSideGeometry;

constexpr int kMaxBlockLds = 160 * 1024;       // gfx950: 160 KiB per CU, one block may take it all
static_assert(kSideTileLdsBudget < kMaxBlockLds, "the side tile's LDS budget leaves a margin inside a CU's LDS");
constexpr int kSlots = 4;                      // staging slots of the host-pointer pipeline
constexpr int kDefaultBlockLds = 64 * 1024;    // above this the kernel attribute must be raised

struct LaunchPlan {
    bool long_mode = false;        // sequences too long for one register sweep / LDS-resident reference
    const Geometry *geo = nullptr;
    WaveLds lds{};
    int waves_per_block = 4;
    int pairs_per_wave = 0;
};

// ONE environment variable for tests and experiments -- VALIGN_HIP_DEBUG="name[=value],name[=value],..." -- read when an
// engine is created; production hosts never set it.  Unknown names are refused: a typo must not silently test nothing.
class DebugSwitches {
public:
    DebugSwitches() {
        const char *env = getenv("VALIGN_HIP_DEBUG");
        if (!env) return;
        static const char *const known[] = {"no_sym", "no_tag", "no_f16", "no_max3", "no_tilt", "no_row_tables", "no_side_tile", "no_fused", "no_prof_key", "no_overlap", "no_band_chain",
                                            "force_long", "wide_align", "strip_k", "no_single_strip", "no_direct_out", "ragged_min", "chunk_bytes",
                                            "align_chunk_bytes", "direct_bytes", "scratch_cap_mb", "whole_rows", "short_strips", "cigar_rows_mb", "cigar_lanes",
                                            "span_scratch_bytes", "subopt_scratch_bytes", "span_cigar_mb"};
        std::string s(env);
        for (size_t at = 0; at <= s.size();) {
            const size_t end = std::min(s.find(',', at), s.size());
            const std::string item = s.substr(at, end - at);
            at = end + 1;
            if (item.empty()) continue;
            const size_t eq = item.find('=');
            const std::string name = item.substr(0, eq);
            bool ok = false;
            for (const char *k : known) ok = ok || name == k;
            if (!ok) throw std::runtime_error("VALIGN_HIP_DEBUG: unknown switch '" + name + "'");
            kv_[name] = eq == std::string::npos ? 1 : atoll(item.c_str() + eq + 1);
        }
    }
    bool on(const char *name) const { return kv_.count(name) != 0; }
    long long value(const char *name, long long fallback) const {
        auto it = kv_.find(name);
        return it == kv_.end() ? fallback : it->second;
    }

private:
    std::map<std::string, long long> kv_;
};

}  // namespace valign

#include "host_runtime.hip.h"

namespace valign {

class Engine {
public:
    struct LengthGroup {
        int R = 0, F = 0;               // strides (= swept shape) of the group
        long long pairs = 0, pair_ofs = 0;
        size_t read_ofs = 0, ref_ofs = 0;
    };
    struct HostStats {             // of the last score_host call
        int launches = 0;
        double cells_swept = 0, cells_padded = 0;
        double gather_ms = 0, wait_ms = 0, drain_ms = 0;     // host time: packing, blocked on the device, copy-out
        double classify_ms = 0;                              // length-sorted batching: host time spent waiting for the device's histograms
        double launch_ms = 0;                                // ... and laying the groups out + launching their sweeps
        int packed = 0;                                      // 1: the sequences crossed PCIe as 4-bit classes
        int direct_out = 0;                                  // 1: results were copied straight into the caller's (registered) buffers
        int direct = 0;                                      // 1: small call, kernels worked on the pinned staging directly; 2: ... in one fused launch
        double d2h_row_bytes = 0, full_row_bytes = 0;        // align_host: result-row bytes that crossed PCIe / that whole rows would have been
    };

    Engine(int device, int R, int F, const Scoring &sc, int force_g, int force_k);

    ~Engine();

    // Banded Smith-Waterman scores (strip band of long_kernels.hip.h); 0 = every cell.  Takes the
    // long-read path whatever the shape -- while the band is set: 0 puts the plan chosen at construction back, so an
    // engine whose band was set and cleared plans every call as a new one does.
    void set_band_width(int diagonals) {
        if (diagonals < 0) throw std::runtime_error("band_width must be >= 0");
        band_width_ = diagonals;
        plan_ = (diagonals > 0 && !base_plan_.long_mode) ? long_plan() : base_plan_;
        band_plan_ = band_chain_plan(R_, F_, band_width_, sc_.affine);      // (once per band_width: shape and scoring are the engine's)
    }
    int band_width() const { return band_width_; }
    // Alignments under band_width (opt-in, so that band_width keeps its meaning for existing callers): 1 = compute_alignments
    // returns banded Smith-Waterman alignments on the block band of the scores (band_block_shape; linear and affine gaps,
    // traceback_policy 0), 0 = every cell whatever band_width says (default)
    void set_band_alignments(int on) {
        if (on != 0 && on != 1) throw std::runtime_error("band_alignments must be 0 or 1");
        band_alignments_ = on == 1;
    }
    int band_alignments() const { return band_alignments_ ? 1 : 0; }
    // The band for the NW variant too (opt-in; include/valign_hip.h has the definition): 1 = band_width > 0 also applies to
    // NW-variant scores and, with band_alignments = 1, to NW-variant alignments; 0 = both are refused under a band (default)
    void set_band_nw(int on) {
        if (on != 0 && on != 1) throw std::runtime_error("band_nw must be 0 or 1");
        band_nw_ = on == 1;
    }
    int band_nw() const { return band_nw_ ? 1 : 0; }
    // Placed scores under the band (opt-in; include/valign_hip.h has the definition): 1 = with band_width > 0
    // valign_hip_score_placed_* run on the block chain and return the banded score and its first in-band end cell; 0 = placed
    // scores are refused under a band (default).  Not read without a band.
    void set_band_placed(int on) {
        if (on != 0 && on != 1) throw std::runtime_error("band_placed must be 0 or 1");
        band_placed_ = on == 1;
    }
    int band_placed() const { return band_placed_ ? 1 : 0; }
    // Placed and spanned scores on int32 cells (opt-in; include/valign_hip.h has the definition): 1 = unbanded Smith-Waterman
    // calls that score_width = 32 or the int16 range rule would refuse run on the pointer-free int32 sweep
    // (placed_wide_kernels.hip.h); 0 = they are refused (default).  Calls inside the int16 range keep their routes.
    void set_placed_wide(int on) {
        if (on != 0 && on != 1) throw std::runtime_error("placed_wide must be 0 or 1");
        placed_wide_ = on == 1;
    }
    int placed_wide() const { return placed_wide_ ? 1 : 0; }
    // Extension scores on int32 cells and row strips (opt-in; include/valign_hip.h has the definition): 1 = extension calls that
    // score_width = 32, the int16 range rule or the read length would refuse run on the int32 extension sweep
    // (extend_wide_kernels.hip.h); 0 = they are refused (default).  Calls the register sweep serves keep it.
    void set_extend_wide(int on) {
        if (on != 0 && on != 1) throw std::runtime_error("extend_wide must be 0 or 1");
        extend_wide_ = on == 1;
    }
    int extend_wide() const { return extend_wide_ ? 1 : 0; }
    // Banded extension scores (opt-in; include/valign_hip.h has the definition): 1 = with band_width > 0 valign_hip_score_extend_*
    // run on the int32 extension sweep over the block band on the anchor's diagonal (extend_band_plan.h); 0 = extension calls are
    // refused under a band (default).  Not read without a band, nor by any other call.
    void set_extend_band(int on) {
        if (on != 0 && on != 1) throw std::runtime_error("extend_band must be 0 or 1");
        extend_band_ = on == 1;
    }
    int extend_band() const { return extend_band_ ? 1 : 0; }
    // Banded extension alignments (opt-in; include/valign_hip.h has the definition): 1 = with band_width > 0 and extend_band = 1
    // valign_hip_align_extend_* run banded on the int32 strip sweep with back pointers (extend_band_align_kernels.hip.h); 0 = they
    // are refused under a band (default).  Not read without a band or without extend_band, nor by any other call.
    void set_extend_band_align(int on) {
        if (on != 0 && on != 1) throw std::runtime_error("extend_band_align must be 0 or 1");
        extend_band_align_ = on == 1;
    }
    int extend_band_align() const { return extend_band_align_ ? 1 : 0; }
    // Z-drop of extension scores and alignments (opt-in; include/valign_hip.h has the definition, extend_zdrop.h the rule): Z > 0 =
    // valign_hip_score_extend_* and valign_hip_align_extend_* stop counting rows at the first row that drops under Z, on the int32
    // strip sweep's ZDROP instances; 0 = every row counts (default).  No other call reads it.
    void set_extend_zdrop(int Z) {
        if (!extend_zdrop_key_ok(Z)) throw std::runtime_error(kExtendZdropKeyRange);
        extend_zdrop_ = Z;
    }
    int extend_zdrop() const { return extend_zdrop_; }
    // The Z-drop on the int16 register sweep (opt-in; include/valign_hip.h has the definition, extend_zdrop.h the routes and the
    // rule's lane form): 1 = unbanded extension calls under extend_zdrop > 0 run the register sweep's ZDROP instances wherever the
    // call without extend_zdrop runs the register sweep; 0 = they run as extend_zdrop alone says (default).  Read by
    // valign_hip_score_extend_* and valign_hip_align_extend_* only, and only where extend_zdrop > 0 and band_width = 0.
    void set_extend_zdrop_rows(int on) {
        if (!extend_zdrop_rows_key_ok(on)) throw std::runtime_error(kExtendZdropRowsKeyRange);
        extend_zdrop_rows_ = on == 1;
    }
    int extend_zdrop_rows() const { return extend_zdrop_rows_ ? 1 : 0; }
    // Checkpointed traceback of long-read alignments (opt-in; ckpt_plan.h): 1 = calls that take the plain row strips (unbanded,
    // int16 cells, traceback_policy 0; both algorithms, linear and affine gaps) keep one boundary row per strip and ONE strip's
    // pointer region instead of every pointer, and re-fill strip after strip along the walk -- identical results, a scratch that
    // grows with R + F instead of R x F.  Every other call (int32 cells, bands, traceback_policy 1, the register and fused
    // paths) runs exactly as with 0 (default); ran_align_fill says which path ran.
    void set_trace_checkpoints(int on) {
        if (on != 0 && on != 1) throw std::runtime_error("trace_checkpoints must be 0 or 1");
        trace_checkpoints_ = on == 1;
    }
    int trace_checkpoints() const { return trace_checkpoints_ ? 1 : 0; }
    // The block band of banded SW scores and alignments: (16, 1) on the block chain, else (160, 4) (valign_hip.h)
    void band_block_shape(int &block_rows, int &col_align) const;
    // DP cell width of score_alignments: 0 = int16 unless the shape could overflow it (default),
    // 16 = int16 or refuse, 32 = always int32 (strip path, half the throughput)
    void set_score_width(int bits) {
        if (bits != 0 && bits != 16 && bits != 32) throw std::runtime_error("score_width must be 0, 16 or 32");
        score_width_ = bits;
    }
    // 0: Default/OpenCL kernel tie-breaks (default); 1: SSE2/AVX2 kernel tie-breaks
    void set_traceback_policy(int policy) {
        if (policy != 0 && policy != 1) throw std::runtime_error("traceback_policy must be 0 (default) or 1 (sse)");
        sse_policy_ = policy == 1;
    }
    // Length-sorted batching of score calls (both modes), done on the device -- classification, packing by length class,
    // one sweep per read class (ragged_kernels.hip.h): 0 = never (every pair is swept at read_length x ref_length; default),
    // 1 = when the call is ragged enough to skip a third of the cells (host pointers: judged from a sample of the call's
    // tails; device-resident batches: from the device's own histogram, which the call then waits for), 2 = always
    void set_ragged_batching(int mode) {
        if (mode < 0 || mode > 2) throw std::runtime_error("ragged_batching must be 0, 1 or 2");
        ragged_ = mode;
    }
    // 4-bit base classes instead of ASCII on the host-pointer score path (host_pipeline.h / pack_kernels.hip.h): 1 on
    // (default), 0 off.  Identical scores; half the bytes across PCIe.
    void set_host_packing(int mode) {
        if (mode != 0 && mode != 1) throw std::runtime_error("host_packing must be 0 or 1");
        pack_ = mode == 1;
    }
    // Half-float cells for score_alignments where they are exact (identical scores, fewer instructions): 1 on (default),
    // 0 integer cells only (what BASELINE.json's "int16" headline is measured with)
    void set_half_float_cells(int mode) {
        if (mode != 0 && mode != 1) throw std::runtime_error("half_float_cells must be 0 or 1");
        no_f16_ = mode == 0 || dbg_.on("no_f16");
    }
    // Cap of the internal pointer scratch of compute_alignments in MiB (0: 64 GiB / half the free HBM); batches
    // that need more run in chunks.  The environment's VALIGN_HIP_SCRATCH_CAP_MB (test switch) applies when this is 0.
    void set_pointer_scratch_cap_mb(long long mb) {
        if (mb < 0) throw std::runtime_error("pointer_scratch_cap_mb must be >= 0");
        if (mb > 0) scratch_cap_mb_ = mb;
    }
    int device() const { return device_; }
    int read_length() const { return R_; }
    int ref_length() const { return F_; }
    const LaunchPlan &plan() const { return plan_; }
    hipStream_t own_stream() const { return streams_[0].get(); }

    // Device-resident batch, asynchronous on `stream`.
    // `length_sorted` false: the caller has decided about length-sorted batching itself (the chunk pipeline of score_host)
    void score_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs,
                      int16_t *d_scores, hipStream_t stream, bool length_sorted = true);

    // One launch of the register-sweep score kernel over n pairs of shape R x F (sequences laid
    // out pair-major at exactly those strides) with the geometry of `plan`.
    // `groups` (length-sorted batches): packed groups sharing the read stride R, each with its own
    // reference stride <= F, swept by one launch; offsets are relative to d_reads / d_refs / d_scores.
    void launch_score(const LaunchPlan &plan, int alg, int R, int F, long long n, const uint8_t *d_reads,
                      const uint8_t *d_refs, int16_t *d_scores, hipStream_t stream,
                      const LengthGroup *groups = nullptr, int n_groups = 0);


    // n sequences of `len` 4-bit classes -> n * len canonical bytes (pack_kernels.hip.h)
    void launch_unpack(const uint8_t *d_packed, uint8_t *d_out, long long n, int len, hipStream_t stream);

    // ---- long reads (engine_long.hip; long_plan.h decodes the route, sizes the strips and plans the chain) ----
    // What long_score_mode reads of this engine beyond the rule inputs, and the route of a score call of `alg` that takes the
    // long-read path.  refuse: throw what the call refuses; false: the route it would have taken (describe, score_host)
    LongFacts long_facts(int alg) const {
        return LongFacts{band_width_, band_nw_, score_wide_cells(alg), dbg_.on("short_strips"), dbg_.on("no_single_strip"), no_band_chain_, band_plan_.usable};
    }
    LongScoreMode long_mode(int alg, bool refuse) const { return long_score_mode(rule_inputs(), alg, long_facts(alg), refuse); }

    // Row strips of the mode's G * K rows, boundary rows through an HBM scratch -- or, banded, the block chain.
    void score_long_device(int alg, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int16_t *d_scores, hipStream_t stream);
    // Banded scores (SW and, under band_nw, the NW variant; linear and affine gaps) on the cyclic block chain of
    // band_kernels.hip.h, for a mode whose route is the chain; its tables follow band_width_ (sync_band_tables).  d_placed:
    // placed scores under band_placed = 1 (engine_placed.hip) -- the same launch with the kernel's PLACED form, records
    // instead of d_scores
    void sync_band_tables(hipStream_t stream);
    void score_band_device(const LongScoreMode &mode, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int16_t *d_scores, PlacedRec *d_placed,
                           hipStream_t stream);

    // The cell format score_alignments is PREDICTED to compute in for this mode: a device-resident call of n pairs (n <= 0:
    // a large call) at the engine's full shape.  What a call really launched is ran_score_cells(): the host pipeline's
    // chunks may be small enough for the latency plan, and length-sorted batches sweep each length class on a plan of its own.
    const char *score_cell_format(int alg, long long n = 0) const;
    // what the last score / alignment call launched (describe: ran_score_cells, ran_align_fill, ran_score_geometry,
    // ran_align_geometry)
    std::string ran_score_cells() const;
    const char *ran_align_fill() const { return ran_align_fill_; }
    static std::string ran_geometry(const Geometry *g) { return g ? std::to_string(g->G) + "x" + std::to_string(g->K) : "none"; }
    std::string ran_kernels() const;

    // What the pure rules of cell_rules.h read of this engine
    RuleInputs rule_inputs() const {
        RuleInputs in = RuleInputs{sc_, R_, F_, sse_policy_, no_sym_, no_tag_, no_f16_, no_prof_key_, no_max3_, no_tilt_};
        in.no_row_tables = no_row_tables_;
        in.no_side_tile = no_side_tile_;
        return in;
    }
    // score_alignments at the engine's full shape stays inside int16 cells (int16_range_ok with this engine's plans: the
    // NW variant's tilt over the tallest register sweep a call may take)
    bool score_int16_ok(int alg) const;
    bool score_wide_cells(int alg) const { return score_width_ == 32 || (score_width_ == 0 && !score_int16_ok(alg)); }

    // Host pointers in, host scores out.  Chunked over kSlots pinned slots, each with its own
    // stream: while the kernel of chunk c runs, chunk c+1 crosses PCIe and the host threads gather
    // chunk c+2 (two slots would serialise copy and kernel of a chunk behind the gather).
    //
    // Smith-Waterman chunks are length-sorted on the way (the reference pads
    // every sequence to the longest, src/util/versalignUtil.cpp:17-33, and sweeps the padding):
    // trailing bytes that are not ACGT score 0 against everything (DefaultKernel.h:83-97), so with
    // gap scores <= 0 no cell of a trailing row or column can exceed the maximum already seen and
    // the SW score of the trimmed pair is the score of the padded one.  Pairs are binned by trimmed
    // (read, ref) length class, each bin is packed at its own strides and swept by the geometry
    // that suits it; scores return through the permutation.  Bit-exact by construction, checked in
    // tests/test_gpu_ragged.py.
    // `d_dest` (the plugin's hip_devices_allgather): the scores stay on the device, pair i at d_dest[i], and `scores` is not
    // touched -- the caller gathers the shards of all devices there (RCCL) before anything goes to the host.
    void score_host(int opt, int n, const char *const *reads, const char *const *refs, short *scores,
                    int threads, int16_t *d_dest = nullptr);


    // ---- compute_alignments ----

    // Device-resident batch -> rows (n * 2 * (R+F) bytes: read row then ref row, right-justified,
    // zero before the start, NUL at R+F-1) and idx (n * 4 shorts).  Asynchronous on `stream`;
    // the pointer scratch is reused chunk after chunk in stream order.
    // `chain` (the chunk pipeline of align_host): the batch is ONE chunk of a sequence of calls.  Its traceback then runs on
    // the engine's helper stream behind the fill, in region `chain->region` (0 / 1) of a pointer scratch sized for two chunks
    // of `chain->chunk_pairs` pairs, and `stream` does NOT wait for it -- the fill of the next chunk (other region) runs
    // beside this walk; the caller chains whatever needs the rows behind trace_done(region).  Returns false where the call
    // ran in stream order instead (row strips, a chunk larger than half the scratch cap): everything is then on `stream`.
    struct WalkChain {
        int region;
        long long chunk_pairs;
        int *min_start;             // device word: the traceback leaves the chunk's smallest readStart there (or nullptr)
        uint8_t *packed;            // ... and the rows, packed to their columns from there on, go here (compact_rows_kernel)
    };
    hipEvent_t trace_done(int region) const { return trace_done_[region].get(); }
    const LaunchPlan &align_plan_for(int alg, FillChoice &choice);
    // The plan compute_alignments starts from: the engine's own -- unless that is the long-read one only because the score
    // kernels prefer it (a reference that starves LDS) while the read fits a register sweep with two waves per CU or so:
    // row strips are 512 rows tall, 150-row reads fill a third of them (150 x 4 000: 1.06 TCUPS on strips).
    const LaunchPlan &align_base_plan() const {
        if (plan_.long_mode && align_resident_.geo && !align_resident_.long_mode && R_ <= 1024 && align_resident_.lds.total <= 140 * 1024) {
            const int wpb = align_resident_.waves_per_block;
            const int waves_per_cu = (kMaxBlockLds / std::max(1, align_resident_.lds.total * wpb)) * wpb;
            if (waves_per_cu >= 2 || !sc_.affine) return align_resident_;      // (150 x 8 000 affine, one wave per CU: 60 ms against 53 on strips)
        }
        return plan_;
    }

    bool align_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, uint8_t *d_rows,
                      short *d_idx, hipStream_t stream, const WalkChain *chain = nullptr);

    void ensure_trace_stream();

    // What align_route (cell_rules.h: the path of an alignment call) reads of this engine.  small_call: the direct call of
    // align_host, which may take the fused kernel
    RouteFacts route_facts(bool small_call) const;

    // Fill + traceback of a small batch in one launch (AlignRoute::Fused): false when no fused geometry holds the shape's
    // pointer stream in LDS (the caller takes the three-kernel path).
    bool align_fused(int alg, long long n, const uint8_t *d_reads, const uint8_t *d_refs, uint8_t *d_rows, short *d_idx,
                     hipStream_t stream);

    // Reads beyond one register sweep: row strips of 64 * K rows, one launch per strip in stream order, boundary
    // rows ping-pong through HBM, one pointer region per strip, then the same traceback kernel (strip_kernels.hip.h).
    // Linear or affine gaps, Default tie-breaks, int16 cells (the reference's; where they would wrap, align_route
    // takes the int32 cells instead of wrapping silently).  mode (strip_plan.h, from the route) -- band: each strip sweeps its
    // rows' band windows only; ckpt: checkpointed traceback (ckpt_plan.h has the schedule): a forward pass without pointers that
    // keeps every strip's bottom row, then per strip, last to first, a re-fill into one pointer region and a resumable walk.
    void align_strips_device(const StripMode &mode, long long n, const uint8_t *d_reads, const uint8_t *d_refs, uint8_t *d_rows, short *d_idx,
                             hipStream_t stream);
    bool align_banded() const { return band_alignments_ && band_width_ > 0; }

    // Host pointers in, Alignment[] out: the rows of every pair are fresh operator new[] blocks
    // (the host's ~Alignment delete[]s them, include/AlignmentKernel.h:20-23).
    // Host pointers in, Alignment[] out.  Three streams: copy-in (H2D), kernels (fill + traceback; they
    // share the pointer scratch, so one stream), copy-out (D2H), chained per chunk with events, over
    // kSlots staging slots -- the 1.3 KB/pair result copy of chunk c, the kernels of chunk c+1 and the
    // input copy of chunk c+2 overlap, and the host gathers / scatters (2n operator new[] blocks, which
    // the ABI demands) meanwhile.
    // `alignments`: the ABI's Alignment array (rows become operator new[] blocks), or a FlatSink (caller-provided
    // contiguous buffers, for FFI callers that do not want 2n heap blocks)
    using FlatSink = valign::FlatSink;      // host_pipeline.h

    template <typename Sink>
    void align_host(int opt, int n, const char *const *reads, const char *const *refs, Sink alignments,
                    int threads);

    // ---- the compact result format (valign_hip.h: valign_hip_aln + ops; engine_cigar.hip) ----
    // Both run the alignment paths above unchanged, into an engine-owned rows scratch (a chunk of the call at a time), and
    // encode each part's rows behind its walk, on the walk's stream, while the part's end cells are still in d_ends_.
    // Device-resident: records and ops at a fixed stride, asynchronous on `stream`.
    void align_cigar_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int extended, CigarRec *d_recs,
                            unsigned *d_ops, int ops_stride, hipStream_t stream);
    // Host pointers: per chunk records on the device (count), an exclusive scan of n_ops, then ops packed at their offsets
    // beside the records (emit) and ONE copy back.  false: the call needs more than ops_cap ops (*ops_needed; recs and
    // offsets are complete).
    bool align_cigar_host(int opt, int n, const char *const *reads, const char *const *refs, int extended, CigarRec *recs,
                          unsigned *ops, long long ops_cap, long long *offsets, long long *ops_needed, int threads);

    // ---- placed Smith-Waterman scores (valign_hip.h: valign_hip_placed; engine_placed.hip) ----
    // Score and end cell of every pair, no traceback: the register sweep with end-cell tracking (placed_kernels.hip.h) or, for
    // reads that take the row strips, the pointer-free forward pass of the checkpointed traceback.  placed_choice
    // (cell_rules.h) decides; what it refuses is thrown.  Device-resident: asynchronous on `stream`, writes d_placed only (the
    // strips keep two boundary row sets and the end cells in an engine-owned scratch between their launches).
    void score_placed_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, PlacedRec *d_placed, hipStream_t stream);
    void score_placed_host(int opt, int n, const char *const *reads, const char *const *refs, PlacedRec *placed, int threads);
    PlacedFacts placed_facts() const;
    const LaunchPlan &placed_plan_for(int alg, PlacedChoice &choice, int &gaps);
    const char *ran_placed() const { return ran_placed_; }

    // ---- spanned Smith-Waterman scores (valign_hip.h: valign_hip_span; engine_span.hip) ----
    // The placed record plus the begin cell: score_placed_device as it stands, the reversal of the prefixes that end in the end
    // cell (span_kernels.hip.h), score_placed_device of a child engine of shape (R, span_ref_length) on the reversed buffers,
    // and the records.  span_choice (cell_rules.h) decides what is refused.  Device-resident: asynchronous on `stream`, in
    // chunks that keep the reversed buffers and the two record buffers inside span_scratch_bytes_; calls of one engine belong
    // on one stream.  Host pointers: record_pipeline, 20 bytes per pair on the way back.
    void score_span_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, SpanRec *d_spans, hipStream_t stream);
    void score_span_host(int opt, int n, const char *const *reads, const char *const *refs, SpanRec *spans, int threads);
    const char *ran_span() const { return ran_span_.c_str(); }

    // ---- spanned CIGARs (valign_hip.h: valign_hip_align_span_*; engine_span_cigar.hip) ----
    // The alignment of the span, filled and walked on the span's window instead of the whole matrix: score_placed_device as it
    // stands, the reversal, align_device of the child engine (shape (R, span_ref_length), every route it has) over the reversed
    // prefixes into an engine-owned rows scratch, and span_cigar_encode_kernel behind its walk, which reads the rows backwards
    // and places the record with the forward one.  span_cigar_choice (cell_rules.h) decides what is refused, before anything is
    // staged or launched.  Device-resident: asynchronous on `stream`, in chunks of whole rounds that keep the reversed
    // prefixes, the forward records and the child's rows inside span_cigar_bytes_; calls of one engine belong on one stream.
    // Host pointers: chunk after chunk on one stream -- gather, H2D, the chunk with a records-only sink, the scan, the emit
    // pass, ONE copy of records and ops back; chunks do not overlap.  false: the call needs more than ops_cap ops.
    void align_span_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int extended, CigarRec *d_recs, unsigned *d_ops,
                           int ops_stride, hipStream_t stream);
    bool align_span_host(int opt, int n, const char *const *reads, const char *const *refs, int extended, CigarRec *recs, unsigned *ops,
                         long long ops_cap, long long *offsets, long long *ops_needed, int threads);
    const char *ran_span_cigar() const { return ran_span_cigar_.c_str(); }

    // ---- suboptimal Smith-Waterman scores (valign_hip.h: valign_hip_subopt; engine_subopt.hip) ----
    // The placed record plus score2 / ref_end2: the placed register sweep in its suboptimal form, which also leaves every
    // column's maximum in an engine-owned scratch, then subopt_records_kernel.  subopt_choice (cell_rules.h) decides what is
    // refused.  Device-resident: asynchronous on `stream`, in chunks of whole rounds that keep the maxima inside
    // subopt_scratch_bytes_; calls of one engine belong on one stream.  Host pointers: record_pipeline, 20 bytes per pair.
    void score_subopt_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int mask, SuboptRec *d_subopt, hipStream_t stream);
    void score_subopt_host(int opt, int n, const char *const *reads, const char *const *refs, int mask, SuboptRec *subopt, int threads);
    const char *ran_subopt() const { return ran_subopt_; }

    // ---- extension scores (valign_hip.h: valign_hip_extend; engine_extend.hip) ----
    // The best score of an alignment anchored before read[0] / ref[0], the cell it ends in, and the best score that consumes the
    // read to its last base: one register sweep with gap-priced borders and no floor (extend_kernels.hip.h), no scratch.
    // extend_choice (cell_rules.h) decides what is refused.  Device-resident: asynchronous on `stream`, writes d_extend only.
    // Host pointers: record_pipeline, 20 bytes per pair.
    void score_extend_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, ExtendRec *d_extend, hipStream_t stream);
    void score_extend_host(int opt, int n, const char *const *reads, const char *const *refs, ExtendRec *extend, int threads);
    const char *ran_extend() const { return ran_extend_; }

    // ---- extension alignments (valign_hip.h: valign_hip_align_extend_*; engine_extend_align.hip) ----
    // The alignment of an extension, from the anchor to the end cell the end-bonus rule picks: align_extend_fill_kernel
    // (extend_align_kernels.hip.h: the extension sweep with a back pointer per cell, which also writes the extension record where
    // d_extend is not null, and the cell the walk starts from), extend_walk_kernel into the CIGAR rows scratch, then the encoder of
    // the compact result format.  extend_align_choice (cell_rules.h) decides what is refused.  Device-resident: asynchronous on
    // `stream`, in chunks that keep the pointer stream under the pointer scratch's cap and the rows under cigar_rows_mb, reused
    // in stream order; calls of one engine belong on one stream.  Host pointers: chunk after chunk on one stream -- gather, H2D,
    // the chunk with a records-only sink, the scan, the emit pass, ONE copy of records, extension records and ops back.
    // false: the call needs more than ops_cap ops.
    void align_extend_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int end_bonus, int extended, CigarRec *d_recs,
                             unsigned *d_ops, int ops_stride, ExtendRec *d_extend, hipStream_t stream);
    bool align_extend_host(int opt, int n, const char *const *reads, const char *const *refs, int end_bonus, int extended, CigarRec *recs, unsigned *ops,
                           long long ops_cap, long long *offsets, long long *ops_needed, ExtendRec *extend, int threads);
    const char *ran_extend_align() const { return ran_extend_align_; }

    // host-side phases of the last score_host / align_host call
    std::string host_phases() const;

    std::string describe(int opt, long long n) const;

private:
    void validate_scoring();

    // the eight scoring fields every kernel argument struct carries under these names
    template <class A>
    void put_scoring(A &a) const {
        a.match = (short)sc_.match;
        a.mismatch = (short)sc_.mismatch;
        a.gap_read = (short)sc_.gap_read;
        a.gap_ref = (short)sc_.gap_ref;
        a.open_read = (short)sc_.open_read;
        a.ext_read = (short)sc_.ext_read;
        a.open_ref = (short)sc_.open_ref;
        a.ext_ref = (short)sc_.ext_ref;
    }

    // what FillArgs, StripArgs and TraceArgs share: the sequences and the size of the launch's part of the batch, the blocks of
    // its sweep, the scoring -- and, for the two that fill (lds given), the LDS layout of a wave
    template <class A>
    void put_sweep(A &a, const uint8_t *d_reads, const uint8_t *d_refs, long long n, int blocks8) const {
        a.reads = d_reads;
        a.refs = d_refs;
        a.n = n;
        a.R = R_;
        a.F = F_;
        a.blocks8 = blocks8;
        put_scoring(a);
    }
    template <class A>
    void put_lds(A &a, const WaveLds &lds) const {
        a.prof_area = lds.prof_area;
        a.refc_stride = lds.refc_stride;
        a.wave_lds = lds.total;
    }
    template <class A>
    void put_sweep(A &a, const uint8_t *d_reads, const uint8_t *d_refs, long long n, int blocks8, const WaveLds &lds) const {
        put_sweep(a, d_reads, d_refs, n, blocks8);
        put_lds(a, lds);
    }
    // What every strip launch shares (align_strips_device adds ptr and walk): `n` pairs of a chunk, strip `s` of the plan, the
    // boundary row sets it reads (top) and writes (bottom) at dword offsets into `scratch`, the F rows f_rows behind the H rows
    StripArgs strip_args(const uint8_t *d_reads, const uint8_t *d_refs, long long n, const StripPlan &plan, const WaveLds &lds, int s, unsigned *scratch,
                         size_t top, size_t bottom, size_t f_rows, EndCell *ends, const int *first_bad) const {
        StripArgs a{};
        put_sweep(a, d_reads, d_refs, n, plan.blocks8, lds);
        a.ends = ends;
        a.first_bad = first_bad;
        a.top = scratch + top;
        a.bottom = scratch + bottom;
        a.top_f = a.top + f_rows;           // (only read / written by the affine kernel)
        a.bottom_f = a.bottom + f_rows;
        a.strip = s;
        a.strips = plan.strips;
        a.row_dwords = plan.row_dwords;
        a.band = plan.band;
        return a;
    }
    // The pointer-free strip sweep of PlacedRoute::Strip and PlacedRoute::Wide, of placed and of extension scores: what differs
    // between them is this description.
    struct PlacedSweep {
        // a step of a chunk outside its strips: `a` = the chunk's StripArgs of strip 0 (sequences, count, scratch pointers),
        // `begin` = the chunk's first pair of the call
        using ChunkStep = std::function<void(const StripArgs &a, long long begin, hipStream_t stream)>;
        const void *fn;             // the strip kernel
        WaveLds lds;
        StripPlan plan;
        bool first_bad;             // the kernel takes a first-invalid table (int16 strips: zeros, read by the NW variant only)
        const char *rows_label, *what;      // names of the boundary-row allocation and of the launch, in errors
        ChunkStep close;            // after the strips: the merged per-pair scratch -> the call's records (placed scores: one of the two record kernels)
        size_t pair_bytes = sizeof(EndCell);        // the merged per-pair scratch behind StripArgs.ends: an EndCell, or ...
        // ... extension scores: a partial record and the trimmed lengths, which `bind` points StripArgs.ptr / .first_bad at (`pairs`:
        // those the scratch is sized for) and `open` fills before the chunk's first strip
        std::function<void(StripArgs &a, long long pairs)> bind;
        ChunkStep open;
    };
    PlacedSweep placed_strip_sweep(PlacedRec *d_placed) const;        // int16 cells: the forward pass of the checkpointed traceback (engine_align.hip)
    PlacedSweep placed_wide_sweep(PlacedRec *d_placed) const;         // placed_wide = 1: the int32 sweep, 8 rows per lane (engine_placed.hip)
    // what closes a chunk of placed scores: placed_records_kernel, or placed_wide_records_kernel (wide), into d_placed (engine_placed.hip)
    PlacedSweep::ChunkStep placed_records_step(PlacedRec *d_placed, bool wide) const;
    // extend_wide = 1: the int32 extension sweep, 8 rows per lane; banded: its form over the band of extend_band = 1 (engine_extend.hip)
    PlacedSweep extend_wide_sweep(ExtendRec *d_extend, bool banded = false) const;
    // its banded form without a record sink: the plan, the LDS, the scratch binding and the lengths pre-pass that banded extension
    // alignments share with the scores (engine_extend_align.hip launches its own fill and closes the chunk itself)
    PlacedSweep extend_band_sweep() const;
    // extend_zdrop > 0: the counter of skipped waves, zeroed on the call's stream when an extension call starts (engine_extend.hip);
    // read back by describe() ("extend_zdrop_skipped_waves"; waits for the device)
    void start_extend_zdrop(hipStream_t stream);
    long long extend_zdrop_skipped_waves() const;
    // Chunk after chunk of what the scratch cap holds: strip after strip through two boundary row sets that ping-pong, the per-pair
    // scratch merged on the way, then the description's records.  The scratch is the engine's, shared by every description.
    void score_placed_strips(const PlacedSweep &sweep, long long n, const uint8_t *d_reads, const uint8_t *d_refs, hipStream_t stream);
    // a block of more than the default LDS: the kernel's attribute first
    static void raise_block_lds(const void *fn, int bytes) {
        if (bytes > kDefaultBlockLds)
            hip_check(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes), "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    }
    TraceArgs trace_args(int alg, const uint8_t *d_reads, const uint8_t *d_refs, long long n, const unsigned *ptr, const EndCell *ends, uint8_t *rows,
                         short *idx, int G, int K, int pad_rows, int blocks8) const;

    // latency: pick for the shortest single sweep (few pairs: every wave has a SIMD to itself and the call takes
    // as long as one wave does) instead of for the most cell updates per second
    LaunchPlan choose_plan(int R, int F, int force_g, int force_k, bool latency = false, bool full_only = false) const;

    static LaunchPlan long_plan();

    // The plan of one register-sweep SCORE launch of `alg` over R x F: `base` (the engine's, the latency plan or a length class's),
    // or the 8 x 19 side tile where its rule has nothing to refuse (cell_rules.h: sym_affine_side_tile_refusal).  Every other
    // call of the engine -- alignments, placed, spanned, suboptimal and extension scores, the NW variant -- plans from the
    // geometry table as ever: the side geometry has one kernel.  A FORCED side tile (group_lanes = 8, rows_per_lane = 19)
    // raises the rule's text where it refuses.
    // refuse = false (describe): what the launch WOULD take, nothing is raised.
    LaunchPlan score_plan_for(const LaunchPlan &base, int alg, int R, int F, bool latency, bool refuse = true) const;
    static LaunchPlan side_plan(int R, int F);
    const char *side_tile_refusal(int alg, int R, int F, bool latency) const;
    // a device-resident score call of n pairs is small enough for the latency plan (score_device and describe share it)
    bool few_pairs(long long n) const { return n > 0 && n <= (long long)latency_plan_.pairs_per_wave * 1024 && band_width_ == 0; }
    // The forms the 8 x 19 launches of the last score call ran, read back from the device (waits for it): "row_tables",
    // "row_tables_repair", "both", or "none" where no wave of such a launch has run
    const char *ran_side_tile_form() const;
    void reset_side_tile_form(hipStream_t stream);      // stream null: synchronously (the host pipeline, whose chunks run on several streams)


    // A chunk of the host-pointer pipeline is one kernel launch: sized in whole "rounds" of the waves the device runs side by
    // side (16,384 pairs at 16 x 10: 8 pairs per wave, 8 waves per CU, 256 CUs), it leaves no partly filled last round --
    // a 48 MB chunk of 150 x 500 was 4.57 rounds and paid for 5.
    // sw_scores: the chunk is one of a Smith-Waterman SCORE call, whose launches take the 8 x 19 side tile where its rule holds:
    // whole rounds of that plan too (32,768 pairs at 150 x 500, a multiple of 16 x 10's 16,384).  Every other call rounds as ever.
    long long whole_rounds(long long pairs, bool sw_scores = false) const;

    // Small calls skip the chunk pipeline (VALIGN_HIP_DIRECT_BYTES: sequence bytes up to which they do; 0 = never)
    bool direct_call(long long n, size_t per_pair) const;

    // Input copies (H2D) and result copies (D2H) of align_host must not share an SDMA engine: 0.65 GB in and 1.36 GB out
    // per million pairs of 150 x 500 would queue up behind each other (36 ms of copying beside 28 ms of kernels).
    // The runtime gives a stream the lowest-numbered engine that is FREE at the stream's first copy and keeps it there
    // (AMD_LOG_LEVEL=4: "Last copy mask 0x1" on both streams, profiles/r03_copy_engines.txt) -- and at the start of a
    // pipeline the first result copy finds the input engine idle.  So, once per engine: a small result copy is issued
    // while a long input copy keeps engine 0 busy, which lands the result stream on the next engine for good.  No
    // API promises this; where it does not work the only loss is the overlap.
    void prime_copy_engines(hipStream_t copy_in, hipStream_t copy_out, long long staged_pairs);

    // the caller's result buffers, when they can take the device's copies directly (page-locked, contiguous)
    void flat_destination(FlatSink sink, long long n, uint8_t *&rows, short *&idx) const {
        if (HostRegistry::instance().covers(sink.rows, (size_t)n * 2 * sink.AL) &&
            HostRegistry::instance().covers(sink.idx, sizeof(short) * 4 * (size_t)n)) {
            rows = sink.rows;
            idx = sink.idx;
        }
    }
    template <typename AlignmentT>
    void flat_destination(AlignmentT *, long long, uint8_t *&, short *&) const {}      // 2n heap rows: always scattered

    // device-side address of pinned host memory of this engine (hipHostMalloc: mapped, same address on ROCm)
    static uint8_t *dev_view(void *pinned) {
        void *d = nullptr;
        hip_check(hipHostGetDevicePointer(&d, pinned, 0), "hipHostGetDevicePointer");
        return (uint8_t *)d;
    }

    // A call that threw in the middle of the pipeline (a HIP error, `too many length groups`) leaves chunks
    // pending in the slots; draining them into the NEXT caller's arrays would write at the old offsets.  Every
    // host-pointer call starts from idle streams and empty slots.
    void reset_pipeline();

    // The pointer stream's bytes per pair-of-pairs depend on the fill kernel the call selects (tagged /
    // untagged, 4- or 8-step blocks, one or two code words): capacity is tracked in BYTES, so a call with a
    // wider stream than the one that sized the scratch reallocates instead of writing past it.
    void ensure_trace_scratch(long long pairs, size_t bytes_per_pp, long long ppw, hipStream_t stream);

    void ensure_align_staging(long long pairs);

    // Where the records (and, device API, the ops) of the alignment call in progress go: set by the two cigar entry points
    // around their align_device / align_fused calls, null otherwise.  Pair 0 of the call is recs[0].
    struct CigarSink {
        CigarRec *recs;
        unsigned *ops;              // null: records only (host path: the ops follow the chunk's scan)
        int ops_stride, extended;
        const PlacedRec *fwd = nullptr;     // not null (the child engine of a spanned CIGAR call): the rows are those of the reversed
        int fwd_ref_length = 0;             // prefixes -- the backward encoder places them with these forward records of an R x fwd_ref_length pair
    };
    // sets an engine's sink for the time of an alignment call and clears it when the call leaves, however it leaves
    struct ScopedSink {
        const CigarSink *&slot;
        ScopedSink(const CigarSink *&s, const CigarSink *value) : slot(s) { slot = value; }
        ~ScopedSink() { slot = nullptr; }
    };
    // encode `cnt` pairs from pair `begin` of the call on `stream`: rows / idx / ends are those of pair `begin`
    void launch_cigar(hipStream_t stream, const uint8_t *rows, const short *idx, const EndCell *ends, long long begin, long long cnt);
    // cigar_encode_kernel over rows of `pitch` bytes (R + F behind an alignment's walk, R + F + 1 behind an extension's); any pass:
    // the caller fills what this leaves open
    void launch_cigar_args(hipStream_t stream, CigarArgs &a, int pitch);
    // The encoders' lane group per pair, for every encoder launch (launch_encoder is the only caller): 16 lanes where an
    // alignment is a few steps of 16 columns (short reads: ~160 columns at 150 x 500), a wave beyond that (measured).
    // Debug switch cigar_lanes forces one.  The answer is noted for describe() ("ran_cigar_lanes").
    int take_cigar_lanes() {
        int lanes = std::min(R_, F_) <= 256 ? 16 : 64;
        const long long forced = dbg_.value("cigar_lanes", 0);
        if (forced == 16 || forced == 64) lanes = (int)forced;
        ran_cigar_lanes_ = lanes;
        return lanes;
    }
    // the scoring fields CigarArgs and SpanCigarArgs carry under these names (ints, and the gap form beside them)
    template <class A>
    void put_cigar_scoring(A &a) const {
        a.affine = sc_.affine ? 1 : 0;
        a.match = sc_.match;
        a.mismatch = sc_.mismatch;
        a.gap_read = sc_.gap_read;
        a.gap_ref = sc_.gap_ref;
        a.open_read = sc_.open_read;
        a.ext_read = sc_.ext_read;
        a.open_ref = sc_.open_ref;
        a.ext_ref = sc_.ext_ref;
    }
    // The one encoder launch: `a` with its rows, sinks, count and pitch set; the scoring, the lane group (k16 / k64: the kernel's
    // two instances) and the grid are decided here.  `what` names the launch in an error.
    template <class A>
    void launch_encoder(hipStream_t stream, A &a, void (*k16)(const A), void (*k64)(const A), const char *what) {
        put_cigar_scoring(a);
        const int lanes = take_cigar_lanes();
        const long long per_block = 256 / lanes;
        const long long blocks = (a.n + per_block - 1) / per_block;
        if (blocks > 0x7FFFFFFFll) throw std::runtime_error("batch too large for one launch");
        hipLaunchKernelGGL(lanes == 16 ? k16 : k64, dim3((unsigned)blocks), dim3(256), 0, stream, a);
        hip_check(hipGetLastError(), what);
    }
    void ensure_cigar_scratch(int slots, long long pairs, hipStream_t stream);
    // offsets[0 .. n] = exclusive scan of recs[p].n_ops on `stream` (cigar_scan_kernel)
    void launch_cigar_scan(const CigarRec *recs, long long *offsets, long long n, hipStream_t stream);

    // ---- packed delivery (engine_cigar.hip): what the three *_host calls of the compact format do with a chunk, once ----
    // The chunk's count-pass records and scanned offsets on the device, and records + extra records + ops as they cross PCIe
    struct CigarPack {
        DeviceBuffer<CigarRec> recs;
        DeviceBuffer<long long> offsets;
        DeviceBuffer<uint8_t> out;
        PinnedBuffer<uint8_t> h_out;
    };
    // the argument checks of the entry points, before anything else is looked at (texts: include/valign_hip.h)
    static void check_packed_device_args(int extended, int ops_stride, const void *d_recs, const void *d_ops);
    static void check_packed_host_args(int extended, int n, const void *recs, const void *ops, long long ops_cap, const long long *offsets, const long long *ops_needed);
    // pairs of one chunk of a host call before the caller's own bound: chunk_bytes of inputs + results, in whole rounds, at least 1024
    long long packed_chunk_pairs(size_t chunk_bytes) const {
        return std::max<long long>(whole_rounds((long long)(chunk_bytes / ((size_t)3 * (R_ + F_) + 8))), 1024);
    }
    // gather and H2D of the caller's BYTES on `stream`: the chunk lies in d_reads_ / d_refs_[slot].  Not stage_chunk, which sends
    // 4-bit classes under host_packing: alignments report the caller's bytes.
    void stage_raw_chunk(int slot, hipStream_t stream, const char *const *reads, const char *const *refs, long long cnt, int threads);
    // behind a chunk's count pass (records only, into pack.recs) on `stream`: the scan and the op total on its way to *h_total_slot
    void finish_count_pass(CigarPack &pack, long long cnt, long long *h_total_slot, hipStream_t stream);
    // With the chunk's total known: the packed buffers grown to `layout`, the emit pass where the ops still fit --
    // fill_and_launch(ops, recs_out) launches the encoder at pack.offsets, which also copies pack.recs to recs_out --, d_extra (null:
    // none) between them, and ONE copy to pack.h_out on `stream`.  Records alone are copied straight from pack.recs.
    using EmitLaunch = std::function<void(unsigned *ops, CigarRec *recs_out)>;
    void emit_packed(CigarPack &pack, const PackedLayout &layout, const EmitLaunch &fill_and_launch, const void *d_extra, hipStream_t stream);
    // what every emit pass's args share: A = CigarArgs / SpanCigarArgs
    template <class A>
    A emit_args(const CigarPack &pack, const uint8_t *rows, const short *idx, long long cnt, int extended, unsigned *ops, CigarRec *recs_out) const {
        A a{};
        a.rows = rows;
        a.idx = idx;
        a.ops = ops;
        a.offsets = pack.offsets.get();
        a.recs_in = pack.recs.get();
        a.recs_out = recs_out;
        a.n = cnt;
        a.extended = extended;
        return a;
    }
    // pack.h_out (its copy waited for) -> the caller's arrays (HostPacker::unpack_packed), timed as the drain phase
    void drain_packed(const CigarPack &pack, const PackedLayout &layout, long long begin, CigarRec *recs, void *extra, unsigned *ops, long long *offsets,
                      int threads);

    // gather / scatter between the caller's scattered blocks and the staging: host_pipeline.h (host-only, sanitizer-tested)
    template <typename Sink>
    void scatter(Sink sink, long long cnt, const uint8_t *rows, const short *idx, int threads, size_t first_col = 0) {
        packer_.scatter(sink, cnt, rows, idx, threads, first_col);
    }

    void ensure_staging(long long pairs);

    // ---- the pieces of the host-pointer chunk pipeline (engine_score.hip), shared by score_host and record_pipeline ----
    // Pairs of one chunk: score_chunk_bytes_ of sequences -- at least 192 MB where the chunks' launches share a scratch and
    // follow one another on one stream (not under the chunk_bytes debug switch) --, in whole rounds, at least 1024, at most n
    long long host_chunk_pairs(bool shared_scratch, long long n, bool sw_scores = false) const;
    // gather (4-bit classes where host_packing is on), H2D and unpacking on `stream`: the chunk lies in d_reads_ / d_refs_[slot]
    void stage_chunk(int slot, hipStream_t stream, const char *const *reads, const char *const *refs, long long cnt, int threads);
    // the slot's event, then drain(slot): the result of the chunk that used the slot last
    void wait_slot(int slot, const std::function<void(int)> &drain);
    // A host-pointer call that brings one fixed-size record per pair back (placed and spanned scores): the direct small call
    // on the pinned staging, else chunks over the kSlots slots -- wait_slot, stage_chunk, launch, D2H, the slot's event -- on
    // streams_[one_stream ? 0 : slot], and the oldest-first tail.  launch: the kernels of one chunk, all of them on `stream`.
    struct RecordKind {
        size_t bytes;
        const char *label, *d2h;            // names of the device staging and of the copy back, in errors
    };
    using ChunkLaunch = std::function<void(int slot, long long cnt, const uint8_t *d_reads, const uint8_t *d_refs, uint8_t *d_records, hipStream_t stream)>;
    // chunk: host_chunk_pairs(one_stream, n), the caller's, which may have sized a scratch of its own by it
    void record_pipeline(long long n, const char *const *reads, const char *const *refs, void *out, const RecordKind &kind, long long chunk, bool one_stream,
                         int threads, const ChunkLaunch &launch);
    void ensure_record_staging(long long pairs, const RecordKind &kind);

    // ---- spanned scores (engine_span.hip) ----
    // One context per pipeline slot (chunks of different slots are in flight side by side) and one for device-resident calls
    struct SpanCtx {
        long long cap = 0;                     // pairs the buffers hold
        DeviceBuffer<uint8_t> rev_reads, rev_refs;
        DeviceBuffer<PlacedRec> fwd, rev;
        size_t bytes() const { return rev_reads.bytes() + rev_refs.bytes() + fwd.bytes() + rev.bytes(); }
    };
    // refusals (thrown), then the child engine of the reverse sweep, created on the first call; strips: either sweep takes the
    // row strips, whose launches share an engine-owned scratch (one stream)
    Engine &span_prepare(int alg, bool &strips);
    long long span_chunk_pairs(long long n) const;
    void ensure_span_scratch(int c, long long pairs, hipStream_t stream);
    // one chunk, all of it on `stream`: forward sweep, reversal, reverse sweep, records
    void span_chunk(int c, int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, SpanRec *d_spans, hipStream_t stream);
    // span_reverse_kernel on `stream`: the prefixes that end in fwd's end cells, reversed, Fr columns of the reference's
    void launch_span_reverse(long long n, const uint8_t *d_reads, const uint8_t *d_refs, const PlacedRec *fwd, uint8_t *rev_reads, uint8_t *rev_refs,
                             int Fr, hipStream_t stream);

    // ---- spanned CIGARs (engine_span_cigar.hip) ----
    // One context for host-pointer calls and one for device-resident calls: the reversed prefixes, the forward records and the
    // child's rows / idx of one chunk; host path: the chunk's pack and its op total
    struct SpanCigarCtx {
        long long cap = 0;                     // pairs the buffers hold
        DeviceBuffer<uint8_t> rev_reads, rev_refs, rows;
        DeviceBuffer<PlacedRec> fwd;
        DeviceBuffer<short> idx;
        CigarPack pack;
        PinnedBuffer<long long> h_total;
        size_t bytes() const { return rev_reads.bytes() + rev_refs.bytes() + rows.bytes() + fwd.bytes() + idx.bytes(); }
    };
    // refusals (thrown), then the child engine, configured as the parent is for this call
    Engine &span_cigar_prepare(int alg);
    long long span_cigar_chunk_pairs(long long n) const;
    void ensure_span_cigar_scratch(int c, long long pairs, bool host, hipStream_t stream);
    // one chunk, all of it on `stream`: forward sweep, reversal, the child's alignment with `sink` behind its walk
    void span_cigar_chunk(int c, int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, const CigarSink &sink, hipStream_t stream);
    // (of the child) encode `cnt` pairs from pair `begin` of the call behind their walk, or, with filled args, any pass:
    // span_cigar_encode_kernel through launch_encoder
    void launch_span_cigar(hipStream_t stream, const uint8_t *rows, const short *idx, long long begin, long long cnt);
    void launch_span_cigar_args(hipStream_t stream, SpanCigarArgs &a);

    // ---- suboptimal scores (engine_subopt.hip) ----
    // One context per pipeline slot and one for device-resident calls: the column maxima and the placed records of one chunk
    struct SuboptCtx {
        DeviceBuffer<unsigned> colmax;
        DeviceBuffer<PlacedRec> placed;
        size_t bytes() const { return colmax.bytes() + placed.bytes(); }
    };
    // refusals (thrown), then the plan: the base plan where its geometry carries the kernel, else the next full geometry
    LaunchPlan subopt_plan_for(int alg, int mask, PlacedChoice &choice, int &gaps);
    long long subopt_chunk_pairs(const LaunchPlan &plan, long long n) const;
    void ensure_subopt_scratch(int c, const LaunchPlan &plan, long long pairs, hipStream_t stream);
    // one chunk, all of it on `stream`: the sweep, then the records
    void subopt_chunk(int c, const LaunchPlan &plan, int track, int gaps, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int mask,
                      SuboptRec *d_subopt, hipStream_t stream);

    // ---- extension scores (engine_extend.hip) ----
    // refusals (thrown), then the plan: the base plan where its geometry carries the kernel, else the next full geometry
    // (route Wide: the base plan, which nothing launches on)
    const LaunchPlan &extend_plan_for(int alg, int &gaps, PlacedRoute &route);

    // ---- extension alignments (engine_extend_align.hip) ----
    // refusals (thrown), then the plan: the base plan where its geometry carries the fill, else the next full geometry
    const LaunchPlan &extend_align_plan_for(int alg, ExtendAlignChoice &choice);
    // pairs of one chunk of a call of n pairs: the pointer stream under the pointer scratch's cap, the rows under `rows_cap` bytes
    long long extend_align_chunk_pairs(const LaunchPlan &plan, const ExtendAlignChoice &choice, long long n, size_t rows_cap) const;
    // the rows scratch of `slots` slots for `pairs` pairs at the walk's row pitch (R + F + 1)
    void ensure_extend_align_rows(int slots, long long pairs, hipStream_t stream);
    // one chunk, all of it on `stream`: fill, walk, encoder (records at recs, ops at ops where not null)
    void extend_align_chunk(const LaunchPlan &plan, const ExtendAlignChoice &choice, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int end_bonus,
                            int extended, CigarRec *recs, unsigned *ops, int ops_stride, ExtendRec *d_extend, int slot, hipStream_t stream);
    // the scratch of a chunk of `pairs` pairs: the walk's rows, the pointer scratch and end cells and, on the Band route, the
    // boundary rows, partial records and trimmed lengths in the strip scratch extension scores use
    void ensure_extend_align_scratch(const LaunchPlan &plan, const ExtendAlignChoice &choice, long long pairs, hipStream_t stream);
    // the Band route's chunk (extend_band_align = 1): the lengths pre-pass, one fill launch per strip, the ends kernel, the walk
    // and the encoder
    void extend_band_align_chunk(const ExtendAlignChoice &choice, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int end_bonus, int extended,
                                 CigarRec *recs, unsigned *ops, int ops_stride, ExtendRec *d_extend, int slot, hipStream_t stream);

    // ---- length-sorted batching (score_host, Smith-Waterman) ----

    static double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    }

    // Both modes (round 3): rows and columns of trailing non-ACGT bytes score 0 against everything, so every value of the
    // real matrix's last row / last column runs down its diagonal unchanged to the padded matrix's last row / column (gap
    // moves only lose) -- the NW variant's max(0, last column, last row) of the trimmed pair IS that of the padded pair,
    // as the Smith-Waterman maximum is.  Checked on the oracle (tests/test_oracle_golden.py) and on the GPU.
    bool ragged_applies(int alg) const;

    // Share of the padded cells a length-sorted sweep would still visit, from 256 pairs spread over
    // the call: sorting costs the host a pass over every tail, so it has to buy something.
    double sampled_cell_fraction(const char *const *reads, const char *const *refs, long long n) const;

    // Read classes: the row capacities of the compiled geometries below read_length, then
    // read_length itself.  Reference classes: multiples of 64 columns, then ref_length.
    void build_length_classes();

    const LaunchPlan &class_plan(int R, int F);

    static int trimmed_length(const unsigned char *s, int len);

    template <typename Fn>
    void for_ranges(int threads, long long cnt, long long serial_below, Fn fn) {
        packer_.for_ranges(threads, cnt, serial_below, fn);
    }

    // ---- length-sorted batching on the device (ragged_kernels.hip.h) ----
    // One context per pipeline slot (chunks of different slots are in flight side by side) and one for device-resident
    // batches (score_device, on the caller's stream).
    struct RaggedCtx {
        long long cap = 0;                     // pairs the buffers hold
        EventHandle counted;                   // (declared before the buffers: they are freed first)
        DeviceBuffer<uint8_t> reads, refs;     // the packed groups
        DeviceBuffer<int16_t> scores;          // ... and their scores, packed order
        DeviceBuffer<uint16_t> bin;            // length bin of every pair
        DeviceBuffer<int> pos;                 // packed place of every pair
        DeviceBuffer<RaggedPlace> place;       // ... as byte offsets + strides, for the copy kernel
        DeviceBuffer<unsigned> counters;       // bins' pair counts, then the groups' fill cursors
        DeviceBuffer<uint8_t> tables;          // device: group_of_bin[bins] then RaggedGroupDev[groups]
        PinnedBuffer<unsigned> h_counts;       // pinned: the histogram's way to the host
        PinnedBuffer<uint8_t> h_tables;        // pinned: the tables' way to the device
        const uint8_t *src_reads = nullptr, *src_refs = nullptr;      // of the chunk between begin and finish
    };
    static constexpr size_t kRaggedTableBytes = sizeof(uint16_t) * kRaggedMaxBins + sizeof(RaggedGroupDev) * kRaggedMaxGroups;

    int ragged_bins() const { return (int)(read_caps_.size() * ref_caps_.size()); }
    bool ragged_fits(long long n) const {
        return ragged_bins() <= kRaggedMaxBins && read_caps_.size() * (size_t)kMaxScoreGroups <= (size_t)kRaggedMaxGroups &&
               n < 0x7FFFFFFFll;
    }

    void ensure_ragged(int c, long long n);

    // first half: trimmed lengths -> bins, the histogram on its way to the host.  Asynchronous on `stream`.
    void ragged_begin(int c, long long n, const uint8_t *d_reads, const uint8_t *d_refs, hipStream_t stream);

    // Fold bins too small to be worth a launch into the next larger one and lay the groups out: a read class with too few
    // pairs for a launch of its own joins the next read class (bin by bin); inside a class, a reference bin smaller than a
    // few blocks joins the next wider one.  Both dimensions only ever grow, so the padded sweep still covers the pair.
    std::vector<LengthGroup> fold_groups(std::vector<long long> &total, std::vector<int> &group_of_bin) const;

    // second half: waits for the histogram, lays the groups out, then -- asynchronously on `stream` -- packs the pairs by
    // group, sweeps class by class and puts the scores back in the caller's order.  `always` false: false is returned, and
    // nothing launched, where the classes would still visit two thirds of the padded cells or more.
    bool ragged_finish(int c, int alg, long long n, int16_t *d_scores, hipStream_t stream, bool always);

    void gather(const char *const *reads, const char *const *refs, long long cnt, uint8_t *dst_reads,
                uint8_t *dst_refs, int threads) {
        packer_.gather(reads, refs, cnt, dst_reads, dst_refs, threads);
    }

    int device_, R_, F_;
    Scoring sc_;
    bool sse_policy_ = false;
    int band_width_ = 0;
    bool band_alignments_ = false;
    bool band_nw_ = false;
    bool band_placed_ = false;
    bool placed_wide_ = false;
    bool extend_wide_ = false;
    bool extend_band_ = false;
    bool extend_band_align_ = false;
    int extend_zdrop_ = 0;
    bool extend_zdrop_rows_ = false;
    bool ran_extend_zdrop_rows_ = false;                 // the last extension call under Z > 0 ran the register sweep: no strips, no skipped waves
    int ran_extend_zdrop_ = 0;                           // the Z the last extension call ran under, 0 without the key (describe)
    bool trace_checkpoints_ = false;
    int score_width_ = 0;
    int ragged_ = 0, force_g_ = 0, force_k_ = 0;
    size_t score_chunk_bytes_ = 48u << 20;                   // staging chunk of score_host (debug switch chunk_bytes)
    size_t align_chunk_bytes_ = 128u << 20;                  // staging chunk of align_host, inputs + results (debug switch align_chunk_bytes)
    size_t direct_bytes_ = 768u << 10;                       // calls with at most this many sequence bytes run on the pinned staging directly
    long long ragged_min_ = 2048;                             // pairs a length bin needs for its own launch
    std::vector<int> read_caps_, ref_caps_;
    std::vector<unsigned char> read_class_;
    std::vector<unsigned short> ref_class_;
    std::map<std::pair<int, int>, LaunchPlan> class_plans_;
    hipStream_t ragged_dev_stream_ = nullptr;                    // stream (the caller's) of the last device-resident length-sorted call
    HostPacker packer_{R_, F_};                               // (declared after R_ / F_)
    HostStats host_stats_;
    DebugSwitches dbg_;                                       // VALIGN_HIP_DEBUG (tests and experiments only)
    bool no_sym_ = dbg_.on("no_sym");                         // the two-gap kernels always
    bool no_tag_ = dbg_.on("no_tag");   // equality-test pointer kernels for linear alignments
    bool no_f16_ = dbg_.on("no_f16");   // int16 cells for symmetric affine SW too
    bool no_max3_ = dbg_.on("no_max3");   // int16 symmetric affine SW scores on the gap-source form always
    bool no_tilt_ = dbg_.on("no_tilt");   // ... and their biased form in the plain frame always
    bool no_row_tables_ = dbg_.on("no_row_tables");   // ... and their tilted frame on the LDS profile always
    bool no_side_tile_ = dbg_.on("no_side_tile");     // ... and never on the 8 x 19 side geometry
    bool side_forced_ = false;                        // group_lanes = 8, rows_per_lane = 19: score calls run the side tile or raise
    bool no_fused_ = dbg_.on("no_fused");   // small alignment calls as fill + traceback kernels
    bool no_prof_key_ = dbg_.on("no_prof_key");   // compute the SW lane key instead of carrying it in the profile
    bool copy_engines_primed_ = false;
    std::unique_ptr<CopyIssuer> copy_issuer_;
    bool wide_align_ = dbg_.on("wide_align");         // alignments on int32 cells always (align_strip_wide_kernel)
    bool whole_rows_ = dbg_.on("whole_rows");         // result rows cross PCIe whole (A/B of the device-side packing)
    bool no_direct_out_ = dbg_.on("no_direct_out");   // stage + scatter even into registered result buffers
    bool no_overlap_ = dbg_.on("no_overlap");   // tracebacks in stream order behind their fills
    int strip_k_ = (int)dbg_.value("strip_k", 0);                  // rows per lane of the strip alignment kernels (16 / 12 / 8): tests
    long long scratch_cap_mb_ = dbg_.value("scratch_cap_mb", 0);   // small pointer scratch: chunked alignment batches in tests (key: pointer_scratch_cap_mb)
    bool chain_regions_busy_[2] = {false, false};                 // WalkChain: the region's last walk may still be running
    std::string arch_;
    LaunchPlan plan_, latency_plan_;
    LaunchPlan base_plan_;              // plan_ as the constructor chose it: what set_band_width(0) restores
    LaunchPlan align_resident_;         // what choose_plan picked before the score path's preferences for the long-read kernels
    LaunchPlan fallback_plan_;          // alignments that need a kernel only the full geometries carry (align_plan_for)
    long long slot_begin_[kSlots] = {}, slot_pending_[kSlots] = {};
    long long staged_pairs_ = 0, align_staged_pairs_ = 0;
    size_t record_staged_bytes_ = 0;                                     // bytes each slot of the record staging holds
    bool pack_ = true;                                                   // host_packing: 4-bit base classes across PCIe
    BandPlan band_plan_;               // the block chain's plan for band_width_ (set_band_width)
    int band_tables_width_ = -1;       // ... and the band_width whose tables are on the device
    int band_blocks_per_cu_ = 0, band_lds_ = 0;          // of the last block-chain launch (describe)
    int long_strip_rows_ = 0;                            // rows per strip of the last score_long_kernel launch (describe)
    // Cell formats of the score kernels the last score call launched, one bit each (kRanF16 / kRanInt16 / kRanInt32; a
    // length-sorted batch may mix them), and the path + fill kernel of the last alignment call ("none": no call yet, or the
    // call was refused) -- set where the kernel is picked, not re-derived (describe: ran_score_cells, ran_align_fill)
    static constexpr unsigned kRanF16 = 1, kRanInt16 = 2, kRanInt32 = 4;
    unsigned ran_score_cells_ = 0;
    const char *ran_align_fill_ = "none";
    // ... and the (G, K) geometry whose table the kernel pointer was taken from: of the last register-sweep score launch and
    // of the last AlignRoute::Register fill launch (null -- "none" -- before any, and for every other route)
    const Geometry *ran_score_geo_ = nullptr, *ran_align_geo_ = nullptr;
    // ... and likewise of the last placed, suboptimal and extension register sweep (describe: ran_placed_geometry,
    // ran_subopt_geometry, ran_extend_geometry): the forced or planned geometry, or the full one *_plan_for moved the call to
    const Geometry *ran_placed_geo_ = nullptr, *ran_subopt_geo_ = nullptr, *ran_extend_geo_ = nullptr;
    // ... and the form of the last score_kernel<G, K, kAlgSW, kGapAffineSym> launch of the last score call: "max3" / "sources"
    // (describe: ran_score_sym_affine; null -- the key is absent -- where the call launched no such kernel)
    const char *ran_score_sym_affine_ = nullptr;
    const char *ran_score_sym_affine_frame_ = "plain";   // ... and its frame: "tilted" / "plain" (describe: ran_score_sym_affine_frame, beside that key)
    const char *ran_score_sym_affine_scores_ = "lds_profile";   // ... and where its substitution scores came from: "row_tables" / "lds_profile" (ran_score_sym_affine_scores)
    const char *ran_placed_ = "none";                    // what the last placed-score call ran: key / rows / strip / chain / wide (describe)
    std::string ran_span_ = "none";                      // what the last spanned call ran: forward route / reverse route (describe)
    size_t span_scratch_bytes_ = (size_t)dbg_.value("span_scratch_bytes", 256ll << 20);      // device-resident spanned calls: scratch of one chunk
    std::string ran_span_cigar_ = "none";                // what the last spanned CIGAR call ran: forward route / the child's ran_align_fill (describe)
    size_t span_cigar_bytes_ = (size_t)std::max(0ll, dbg_.value("span_cigar_mb", 768)) << 20;      // scratch of one chunk: the spanned scores' 256 MiB + 512 MiB of rows
    const char *ran_subopt_ = "none";                    // what the last suboptimal call ran: key / rows (describe)
    int subopt_ring_cols_ = 0;                           // ... and the columns of a lane group's ring in its sweep
    size_t subopt_scratch_bytes_ = (size_t)dbg_.value("subopt_scratch_bytes", 256ll << 20);      // column maxima of one chunk
    const char *ran_extend_ = "none";                    // what the last extension call ran: rows, wide (describe)
    const char *ran_extend_align_ = "none";              // what the last extension-alignment call ran: rows (describe)
    const Geometry *ran_extend_align_geo_ = nullptr;     // ... and the geometry its fill was taken from (ran_extend_align_geometry)
    long long ran_extend_align_chunks_ = 0;              // ... and the chunks it was cut into (ran_extend_align_chunks)
    const char *ran_result_format_ = "rows";             // of the last alignment call: rows / cigar (describe)
    int ran_cigar_lanes_ = 0;                            // the lane group the last CIGAR call's encoder ran on: 16 / 64, 0 none (describe)
    long long cigar_d2h_bytes_ = 0;                      // what the last align_cigar_host call copied back
    const CigarSink *cigar_ = nullptr;
    long long cigar_pairs_[2] = {0, 0};                  // pairs the cigar scratch of each slot holds
    long long align_ptr_bytes_per_pair_ = 0;             // pointer-stream bytes per pair of the last alignment call's plan (describe)
    long long align_ckpt_bytes_per_pair_ = 0;            // ... and what StripCkpt keeps beside it: checkpoint rows + walk state
    int cu_count_ = 0;
    bool no_band_chain_ = dbg_.on("no_band_chain");      // banded scores on score_long_kernel's strips
    int start_col_[kSlots] = {};                         // per slot: first column of the chunk's rows the copy issuer copied

    // ---- owned HIP objects.  Members are destroyed in reverse order: the streams and events come first here, so that
    // every buffer is freed before the streams and events it was used on. ----
    StreamHandle streams_[kSlots];
    EventHandle slot_done_[kSlots];
    EventHandle in_done_[kSlots], kernels_done_[kSlots];         // align_host: H2D / kernels of the slot's chunk finished
    StreamHandle trace_stream_;                                  // helper stream of align_device (walks beside the next fill)
    EventHandle fill_done_[2], trace_done_[2], entry_ev_;
    EventHandle ragged_dev_done_;                                // end of the last device-resident length-sorted call
    PinnedBuffer<uint8_t> h_reads_[kSlots], h_refs_[kSlots];     // score / alignment staging, kSlots slots
    PinnedBuffer<short> h_scores_[kSlots];
    DeviceBuffer<uint8_t> d_reads_[kSlots], d_refs_[kSlots];
    DeviceBuffer<int16_t> d_scores_[kSlots];
    DeviceBuffer<uint8_t> d_pack_reads_[kSlots], d_pack_refs_[kSlots];     // 4-bit classes as they arrive (score path)
    // compute_alignments: pointer scratch + end cells (device), result staging (both sides)
    DeviceBuffer<unsigned> d_ptr_;
    DeviceBuffer<EndCell> d_ends_;
    DeviceBuffer<int> d_first_bad_;                              // row strips: first invalid read / ref position per pair
    PinnedBuffer<uint8_t> h_rows_[kSlots];
    PinnedBuffer<short> h_idx_[kSlots];
    DeviceBuffer<uint8_t> d_rows_[kSlots];
    DeviceBuffer<short> d_idx_[kSlots];
    DeviceBuffer<uint8_t> d_packed_rows_[kSlots];                // the chunk's rows without their all-zero leading columns
    // compact result format: the rows the walks write (never copied out), per chunk parity; host path: each parity's pack and
    // the two op totals
    DeviceBuffer<uint8_t> d_cig_rows_[2];
    DeviceBuffer<short> d_cig_idx_[2];
    CigarPack cig_pack_[2];
    PinnedBuffer<long long> h_cig_total_;
    DeviceBuffer<ExtendRec> d_extend_align_recs_;                // extension alignments, host path: the chunk's extension records before they join the packed copy
    DeviceBuffer<int> d_min_start_;                              // per slot: first column of the chunk's rows that holds a string
    PinnedBuffer<int> h_min_start_;                              // ... on its way to the host
    // record_pipeline: record staging (placed or spanned records: one host call runs on an engine at a time)
    PinnedBuffer<uint8_t> h_records_[kSlots];
    DeviceBuffer<uint8_t> d_records_[kSlots];
    // placed scores: the strips' boundary rows, end cells and (unread) first-invalid table
    DeviceBuffer<unsigned> d_placed_rows_;
    DeviceBuffer<EndCell> d_placed_ends_;
    DeviceBuffer<int> d_placed_bad_;
    // spanned scores: the reversal scratch, the engine of the reverse sweep
    SpanCtx span_[kSlots + 1];                                   // one per pipeline slot, the last for device-resident calls
    std::unique_ptr<Engine> span_child_;
    SpanCigarCtx span_cigar_[2];                                 // spanned CIGARs: [0] host-pointer calls, [1] device-resident calls
    SuboptCtx subopt_[kSlots + 1];                               // one per pipeline slot, the last for device-resident calls
    DeviceBuffer<unsigned> d_brow_;                              // long-read path: strip boundary rows
    DeviceBuffer<BandBlock> d_band_blocks_;                      // the block chain's tables (band_plan_)
    DeviceBuffer<int> d_band_fill_;
    RaggedCtx rag_[kSlots + 1];                                  // one per pipeline slot, the last for device-resident batches
    DeviceBuffer<unsigned> d_form_seen_;                         // the 8 x 19 kernel's two form words (ScoreArgs::form_seen)
    DeviceBuffer<unsigned> d_zdrop_skipped_;                     // extend_zdrop > 0, its last call: the waves that skipped a strip
    DeviceBuffer<uint8_t> d_read_class_;                         // length -> class tables of the length-sorted batches
    DeviceBuffer<uint16_t> d_ref_class_;
};

}  // namespace valign
