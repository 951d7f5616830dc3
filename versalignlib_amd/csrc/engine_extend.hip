// engine_extend.hip -- Engine: extension scores (include/valign_hip.h: valign_hip_score_extend_*): per pair the best score of an
// alignment that starts at the anchor, before read[0] and ref[0], the cell it ends in, and the best score that consumes the read
// to its last base.  extend_choice (cell_rules.h) decides what is refused; this unit launches score_extend_kernel
// (extend_kernels.hip.h: the rows track's sweep with gap-priced borders and no floor), which writes the records itself -- no
// scratch, one launch per call.  The host-pointer path is record_pipeline (engine_score.hip) with 20-byte records on the way back.
#include "engine.hip.h"

namespace valign {

// The plan of an extension call: the one alignments start from where its geometry carries the kernel, otherwise the cheapest
// full geometry that fits the read.  Throws what the rule refuses.
const LaunchPlan &Engine::extend_plan_for(int alg, int &gaps) {
    const LaunchPlan &base = align_base_plan();
    const PlacedFacts facts = placed_facts();
    RuleInputs in = rule_inputs();
    in.no_f16 = true;                   // int16 cells: the gap form is one of the four integer ones
    const PlacedChoice choice = extend_choice(in, alg, facts, base.geo ? base.geo->G : 0, base.geo ? base.geo->K : 0);
    if (choice.route == PlacedRoute::Refused) throw std::runtime_error(choice.reason);
    gaps = score_gap_form(in, kAlgSW, R_, F_, base.geo->G * base.geo->K);
    if (base.geo->extend(gaps)) return base;
    if (!fallback_plan_.geo) fallback_plan_ = choose_plan(R_, F_, 0, 0, false, true);
    if (fallback_plan_.long_mode || !fallback_plan_.geo->extend(gaps)) throw std::runtime_error("no extension-score kernel for this mode");
    return fallback_plan_;
}

void Engine::score_extend_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, ExtendRec *d_extend, hipStream_t stream) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;          // reference: unsupported mode is a silent no-op
    ran_extend_ = "none";
    ran_extend_geo_ = nullptr;
    int gaps = 0;
    const LaunchPlan &plan = extend_plan_for(alg, gaps);
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ExtendArgs a{};
    a.reads = d_reads;
    a.refs = d_refs;
    a.extend = d_extend;
    a.n = n;
    a.R = R_;
    a.F = F_;
    put_lds(a, plan.lds);
    put_scoring(a);
    const void *fn = plan.geo->extend(gaps);
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

// Host pointers in, host records out: record_pipeline, 20 bytes per pair on the way back.
void Engine::score_extend_host(int opt, int n, const char *const *reads, const char *const *refs, ExtendRec *extend, int threads) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ran_extend_ = "none";
    ran_extend_geo_ = nullptr;
    int gaps = 0;
    (void)extend_plan_for(alg, gaps);          // (refusals leave here, before anything is staged)
    record_pipeline(n, reads, refs, extend, RecordKind{sizeof(ExtendRec), "extension records", "D2H extension records"}, host_chunk_pairs(false, n), false, threads,
                    [&](int, long long cnt, const uint8_t *d_reads, const uint8_t *d_refs, uint8_t *d_records, hipStream_t stream) {
                        score_extend_device(opt, cnt, d_reads, d_refs, (ExtendRec *)d_records, stream);
                    });
}

}  // namespace valign
