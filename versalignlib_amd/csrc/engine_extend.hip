// engine_extend.hip -- Engine: extension scores (include/valign_hip.h: valign_hip_score_extend_*): per pair the best score of an
// alignment that starts at the anchor, before read[0] and ref[0], the cell it ends in, and the best score that consumes the read
// to its last base.  extend_choice (cell_rules.h) decides what is refused and which route runs; this unit launches
// score_extend_kernel (extend_kernels.hip.h: the rows track's sweep with gap-priced borders and no floor), which writes the records
// itself -- no scratch, one launch per call -- or, where the rule answers Wide (extend_wide = 1), hands score_placed_strips
// (engine_placed.hip) the description of the int32 extension sweep (extend_wide_kernels.hip.h): a length pre-pass per chunk, one
// launch per strip, a record kernel.  Where it answers Band (extend_band = 1 under a band) the same description carries the sweep's
// BANDED instances.  The rule is asked through extend_zdrop_choice (extend_zdrop.h), which wraps extend_choice(in, alg, facts, G, K):
// under extend_zdrop > 0 the strip sweep or nothing, and the
// description carries the sweep's ZDROP instances, a drop row per pair behind the trimmed lengths and the counter of skipped waves.
// Under extend_zdrop_rows = 1 the rule is extend_zdrop_rows_choice, which wraps extend_zdrop_choice(in, alg, facts, G, K, Z): an
// unbanded call under Z > 0 that would run the register sweep without Z runs its ZDROP instance (Geometry::extend_zdrop) on the
// same plan, LDS and launch -- the drop is decided in the kernel's epilogue, nothing else changes.
// The host-pointer path is record_pipeline (engine_score.hip), 20-byte records on the way back.
// extend_wide_lengths_kernel and extend_wide_records_kernel (not templates) are defined in this translation unit.
#define VALIGN_TU_EXTEND 1
#include "engine.hip.h"
#include "extend_wide_kernels.hip.h"

namespace valign {

// The plan of an extension call: the one alignments start from where its geometry carries the kernel, otherwise the cheapest
// full geometry that fits the read.  Throws what the rule refuses.
const LaunchPlan &Engine::extend_plan_for(int alg, int &gaps, PlacedRoute &route) {
    const LaunchPlan &base = align_base_plan();
    const PlacedFacts facts = placed_facts();
    RuleInputs in = rule_inputs();
    in.no_f16 = true;                   // int16 cells: the gap form is one of the four integer ones
    const PlacedChoice choice = extend_zdrop_rows_choice(in, alg, facts, base.geo ? base.geo->G : 0, base.geo ? base.geo->K : 0, extend_zdrop_, extend_zdrop_rows_);
    if (choice.route == PlacedRoute::Refused) throw std::runtime_error(choice.reason);
    route = choice.route;
    if (route == PlacedRoute::Wide || route == kPlacedRouteBand) return base;        // (nothing launches on the plan)
    gaps = score_gap_form(in, kAlgSW, R_, F_, base.geo->G * base.geo->K);
    // (a geometry carries the ZDROP form of an instance exactly where it carries the plain one)
    if (base.geo->extend(gaps) && base.geo->extend_zdrop(gaps)) return base;
    if (!fallback_plan_.geo) fallback_plan_ = choose_plan(R_, F_, 0, 0, false, true);
    if (fallback_plan_.long_mode || !fallback_plan_.geo->extend(gaps) || !fallback_plan_.geo->extend_zdrop(gaps)) throw std::runtime_error("no extension-score kernel for this mode");
    return fallback_plan_;
}

void Engine::score_extend_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, ExtendRec *d_extend, hipStream_t stream) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;          // reference: unsupported mode is a silent no-op
    ran_extend_ = "none";
    ran_extend_geo_ = nullptr;
    ran_extend_zdrop_ = 0;
    ran_extend_zdrop_rows_ = false;
    int gaps = 0;
    PlacedRoute route = PlacedRoute::Refused;
    const LaunchPlan &plan = extend_plan_for(alg, gaps, route);
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (route == PlacedRoute::Wide || route == kPlacedRouteBand) {
        start_extend_zdrop(stream);
        score_placed_strips(extend_wide_sweep(d_extend, route == kPlacedRouteBand), n, d_reads, d_refs, stream);
        ran_extend_ = ran_placed_name(route);
        return;
    }
    ExtendArgs a{};
    a.reads = d_reads;
    a.refs = d_refs;
    a.extend = d_extend;
    a.n = n;
    a.R = R_;
    a.F = F_;
    put_lds(a, plan.lds);
    put_scoring(a);
    // keys extend_zdrop > 0 and extend_zdrop_rows = 1 (the route is Rows, so no band is set): the ZDROP instance
    const bool dropping = extend_zdrop_rows_ && extend_zdrop_on(extend_zdrop_);
    a.Z = dropping ? extend_zdrop_ : 0;
    ran_extend_zdrop_ = a.Z;
    ran_extend_zdrop_rows_ = dropping;
    const void *fn = dropping ? plan.geo->extend_zdrop(gaps) : plan.geo->extend(gaps);
    ran_extend_geo_ = plan.geo;
    const long long ppb = (long long)plan.pairs_per_wave * plan.waves_per_block;
    const long long blocks = (n + ppb - 1) / ppb;
    if (blocks > 0x7FFFFFFFll) throw std::runtime_error("batch too large for one launch");
    const int block_lds = plan.lds.total * plan.waves_per_block;
    raise_block_lds(fn, block_lds);
    void *kargs[] = {&a};
    hip_check(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(plan.waves_per_block * kWave), kargs, (size_t)block_lds, stream),
              "hipLaunchKernel(score_extend_kernel)");
    ran_extend_ = ran_placed_name(PlacedRoute::Rows);
}

// extend_wide = 1: the int32 extension sweep.  8 rows per lane; the wide plan's row sets (an int32 row per pair, and an F row
// beside it, affine) -- its padding rows are counted above the read, the kernel puts them below: the strips, the row sets and their
// sizes are the same either way.  The per-pair scratch is the partial record and, behind the records of every pair the scratch
// holds, the two trimmed lengths.
// banded (extend_band = 1 under a band): the BANDED instances on the same plan, scratch and chunks; the band travels as
// StripArgs.band -- half = w of extend_band_plan.h, capped at the unbanded limit -- and the record kernel takes w for the unreached
// read end.
Engine::PlacedSweep Engine::extend_wide_sweep(ExtendRec *d_extend, bool banded) const {
    constexpr int K = kExtendWideK;
    const bool zdrop = extend_zdrop_on(extend_zdrop_);
    const void *plain = banded ? (sc_.affine ? (const void *)&score_extend_wide_kernel<K, true, true> : (const void *)&score_extend_wide_kernel<K, false, true>)
                               : (sc_.affine ? (const void *)&score_extend_wide_kernel<K, true> : (const void *)&score_extend_wide_kernel<K, false>);
    const void *dropping = banded ? (sc_.affine ? (const void *)&score_extend_wide_kernel<K, true, true, false, true> : (const void *)&score_extend_wide_kernel<K, false, true, false, true>)
                                  : (sc_.affine ? (const void *)&score_extend_wide_kernel<K, true, false, false, true> : (const void *)&score_extend_wide_kernel<K, false, false, false, true>);
    const void *fn = zdrop ? dropping : plain;
    PlacedSweep sweep{fn, WaveLds{StripLds<K>::kRing, 0, StripLds<K>::kTotal}, strip_plan(R_, F_, K, StripMode{kAlgSW, sc_.affine, false, true, false, false}, kNoBand),
                      false, "extension-score boundary rows (int32)", "hipLaunchKernel(score_extend_wide_kernel)"};
    // (ZDROP: a drop row per pair behind the lengths, Z in the band's pad -- the sweep has no padding rows above the read -- and the
    // counter of skipped waves where the walk state of the checkpointed strips travels)
    sweep.pair_bytes = sizeof(ExtendRec) + 2 * sizeof(int) + (zdrop ? sizeof(int) : 0);
    const int band_half = banded ? extend_band_half(placed_facts().band_width, R_, F_) : -1;
    if (banded) sweep.plan.band = BandShape{band_half, kExtendBandBlockRows, kExtendBandColAlign, 0};
    if (zdrop) sweep.plan.band.pad = extend_zdrop_;
    const WalkState *skipped = zdrop ? reinterpret_cast<const WalkState *>(d_zdrop_skipped_.get()) : nullptr;
    sweep.bind = [skipped](StripArgs &a, long long pairs) {
        a.ptr = reinterpret_cast<unsigned *>(a.ends);
        a.first_bad = reinterpret_cast<const int *>(a.ptr + (size_t)kExtendWideRecDwords * pairs);
        a.ends = nullptr;
        a.walk = skipped;
    };
    const int R = R_, F = F_;
    sweep.open = [R, F](const StripArgs &a, long long, hipStream_t stream) {
        hipLaunchKernelGGL(extend_wide_lengths_kernel, dim3((unsigned)a.n), dim3(kWave), 0, stream, a.reads, a.refs, a.n, R, F, const_cast<int *>(a.first_bad));
        hip_check(hipGetLastError(), "hipLaunchKernel(extend_wide_lengths_kernel)");
    };
    sweep.close = [d_extend, band_half, zdrop](const StripArgs &a, long long begin, hipStream_t stream) {
        hipLaunchKernelGGL(extend_wide_records_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, (const int *)a.ptr, a.first_bad, d_extend + begin, a.n, band_half,
                           zdrop ? extend_drop_rows(a) : nullptr);
        hip_check(hipGetLastError(), "hipLaunchKernel(extend_wide_records_kernel)");
    };
    return sweep;
}

Engine::PlacedSweep Engine::extend_band_sweep() const { return extend_wide_sweep(nullptr, true); }

// An extension call on the strip sweep starts: what describe() reports of the key, and the counter at zero on the call's stream
void Engine::start_extend_zdrop(hipStream_t stream) {
    ran_extend_zdrop_ = extend_zdrop_;
    ran_extend_zdrop_rows_ = false;
    if (!extend_zdrop_on(extend_zdrop_)) return;
    if (!d_zdrop_skipped_.get()) d_zdrop_skipped_.reserve(sizeof(unsigned), "extend_zdrop skipped waves");
    hip_check(hipMemsetAsync(d_zdrop_skipped_.get(), 0, sizeof(unsigned), stream), "hipMemsetAsync(extend_zdrop skipped waves)");
}

long long Engine::extend_zdrop_skipped_waves() const {
    if (!extend_zdrop_on(ran_extend_zdrop_) || ran_extend_zdrop_rows_) return 0;       // (the register sweep has no strips)
    unsigned waves = 0;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    hip_check(hipMemcpy(&waves, d_zdrop_skipped_.get(), sizeof waves, hipMemcpyDeviceToHost), "hipMemcpy(extend_zdrop skipped waves)");
    return waves;
}

// Host pointers in, host records out: record_pipeline, 20 bytes per pair on the way back.
void Engine::score_extend_host(int opt, int n, const char *const *reads, const char *const *refs, ExtendRec *extend, int threads) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ran_extend_ = "none";
    ran_extend_geo_ = nullptr;
    ran_extend_zdrop_ = 0;
    int gaps = 0;
    PlacedRoute route = PlacedRoute::Refused;
    (void)extend_plan_for(alg, gaps, route);          // (refusals leave here, before anything is staged)
    const bool strips = route == PlacedRoute::Wide || route == kPlacedRouteBand;      // the strips' launches share the boundary rows: one stream, large chunks
    record_pipeline(n, reads, refs, extend, RecordKind{sizeof(ExtendRec), "extension records", "D2H extension records"}, host_chunk_pairs(strips, n), strips, threads,
                    [&](int, long long cnt, const uint8_t *d_reads, const uint8_t *d_refs, uint8_t *d_records, hipStream_t stream) {
                        score_extend_device(opt, cnt, d_reads, d_refs, (ExtendRec *)d_records, stream);
                    });
}

}  // namespace valign
