// engine_subopt.hip -- Engine: suboptimal Smith-Waterman scores (include/valign_hip.h: valign_hip_score_subopt_*): the placed
// record plus the best column maximum outside a window around the end cell -- SSW's score2 / ref_end2 -- from ONE placed sweep.
// subopt_choice (cell_rules.h) decides what is refused and which track runs; this unit launches score_placed_kernel's SUB form
// (placed_kernels.hip.h: the placed sweep with the column maxima riding its lane-to-lane hand-over, out through an LDS ring
// into an engine-owned scratch) and subopt_records_kernel behind it, chunk after chunk in stream order.  The host-pointer path
// is record_pipeline (engine_score.hip) with 20-byte records on the way back.
// subopt_records_kernel (not a template) is defined in this translation unit.
#define VALIGN_TU_SUBOPT 1
#include "engine.hip.h"

namespace valign {

// The plan of a suboptimal call: the placed call's (placed_plan_for), on the next full geometry where the plan's own has no
// suboptimal instance, with the waves of a block refitted to the tables AND the rings (subopt_block_waves, cell_rules.h)
LaunchPlan Engine::subopt_plan_for(int alg, int mask, PlacedChoice &choice, int &gaps) {
    const LaunchPlan &base = align_base_plan();
    const PlacedFacts facts = placed_facts();
    RuleInputs in = rule_inputs();
    in.no_f16 = true;                   // (as placed_plan_for: int16 cells, one of the four integer gap forms)
    choice = subopt_choice(in, alg, facts, base.geo->G, base.geo->K, mask);
    if (choice.route == PlacedRoute::Refused) throw std::runtime_error(choice.reason);
    gaps = score_gap_form(in, kAlgSW, R_, F_, base.geo->G * base.geo->K);
    auto track_of = [](const PlacedChoice &c) { return c.route == PlacedRoute::Key ? kPlacedKey : kPlacedRows; };
    auto with_rings = [](LaunchPlan plan) {
        plan.waves_per_block = subopt_block_waves(plan.lds.total, kSuboptRingBytes, plan.waves_per_block, kMaxBlockLds);
        if (plan.waves_per_block == 0) throw std::runtime_error(kSuboptNoRing);
        return plan;
    };
    if (base.geo->subopt(track_of(choice), gaps)) return with_rings(base);
    if (!fallback_plan_.geo) fallback_plan_ = choose_plan(R_, F_, 0, 0, false, true);
    choice = subopt_choice(in, alg, facts, fallback_plan_.geo->G, fallback_plan_.geo->K, mask);
    if (choice.route == PlacedRoute::Refused) throw std::runtime_error(choice.reason);
    if (fallback_plan_.long_mode || !fallback_plan_.geo->subopt(track_of(choice), gaps)) throw std::runtime_error("no suboptimal-score kernel for this mode");
    return with_rings(fallback_plan_);
}

// dwords of a pair of pairs' row of column maxima: a multiple of 4, whole 16-byte flushes
static int subopt_col_stride(int F) { return std::max(4, (F + 3) / 4 * 4); }

// Pairs of one chunk: what the scratch holds of column maxima, in whole rounds of the sweep's waves where it holds a round -- a
// round of THIS plan: the blocks a CU holds with their rings, on every CU -- and in whole waves always
long long Engine::subopt_chunk_pairs(const LaunchPlan &plan, long long n) const {
    const size_t per_pp = (size_t)subopt_col_stride(F_) * 4;
    long long chunk = (long long)(subopt_scratch_bytes_ / per_pp) * 2;
    const int block_lds = (plan.lds.total + kSuboptRingBytes) * plan.waves_per_block;
    const long long waves_per_cu = std::min(32, kMaxBlockLds / block_lds * plan.waves_per_block);
    const long long round = std::max<long long>(1, waves_per_cu) * std::max(1, cu_count_) * plan.pairs_per_wave;
    chunk = chunk >= round ? chunk / round * round : std::max<long long>(chunk / plan.pairs_per_wave * plan.pairs_per_wave, plan.pairs_per_wave);
    return std::min(chunk, n);
}

void Engine::ensure_subopt_scratch(int c, const LaunchPlan &plan, long long pairs, hipStream_t stream) {
    SuboptCtx &x = subopt_[c];
    const long long rows = (pairs + plan.pairs_per_wave - 1) / plan.pairs_per_wave * (plan.pairs_per_wave / 2);      // whole waves
    const size_t col_bytes = (size_t)rows * subopt_col_stride(F_) * 4, rec_bytes = sizeof(PlacedRec) * (size_t)pairs;
    if (col_bytes <= x.colmax.bytes() && rec_bytes <= x.placed.bytes()) return;
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");          // nothing may still read the old scratch
    x.colmax.reset();
    x.placed.reset();
    x.colmax.reserve(col_bytes, "suboptimal-score column maxima");
    x.placed.reserve(rec_bytes, "suboptimal-score placed records");
}

void Engine::subopt_chunk(int c, const LaunchPlan &plan, int track, int gaps, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int mask,
                          SuboptRec *d_subopt, hipStream_t stream) {
    SuboptCtx &x = subopt_[c];
    const int stride = subopt_col_stride(F_);
    const long long rows = (n + plan.pairs_per_wave - 1) / plan.pairs_per_wave * (plan.pairs_per_wave / 2);
    if ((size_t)rows * stride * 4 > x.colmax.bytes() || sizeof(PlacedRec) * (size_t)n > x.placed.bytes())
        throw std::runtime_error("suboptimal scores: chunk larger than its scratch");
    SuboptArgs a{};
    a.reads = d_reads;
    a.refs = d_refs;
    a.placed = x.placed.get();
    a.n = n;
    a.R = R_;
    a.F = F_;
    put_lds(a, plan.lds);
    put_scoring(a);
    a.ring_ofs = plan.lds.total;                      // (a multiple of 16: wave_lds)
    a.wave_lds = plan.lds.total + kSuboptRingBytes;
    a.colmax = x.colmax.get();
    a.col_stride = stride;
    const void *fn = plan.geo->subopt(track, gaps);
    ran_subopt_geo_ = plan.geo;
    const long long ppb = (long long)plan.pairs_per_wave * plan.waves_per_block;
    const long long blocks = (n + ppb - 1) / ppb;
    if (blocks > 0x7FFFFFFFll) throw std::runtime_error("batch too large for one launch");
    const int block_lds = a.wave_lds * plan.waves_per_block;             // (within kMaxBlockLds: subopt_plan_for)
    raise_block_lds(fn, block_lds);
    void *kargs[] = {&a};
    hip_check(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(plan.waves_per_block * kWave), kargs, (size_t)block_lds, stream),
              "hipLaunchKernel(score_placed_kernel, suboptimal form)");
    SuboptRecordArgs r{};
    r.refs = d_refs;
    r.placed = x.placed.get();
    r.colmax = x.colmax.get();
    r.subopt = d_subopt;
    r.n = n;
    r.F = F_;
    r.col_stride = stride;
    r.mask = mask;
    const long long rec_blocks = ((n + 1) / 2 + 3) / 4;           // a wave per pair of pairs, four waves per block
    hipLaunchKernelGGL(subopt_records_kernel, dim3((unsigned)rec_blocks), dim3(256), 0, stream, r);
    hip_check(hipGetLastError(), "hipLaunchKernel(subopt_records_kernel)");
}

void Engine::score_subopt_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int mask, SuboptRec *d_subopt, hipStream_t stream) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;          // reference: unsupported mode is a silent no-op
    ran_subopt_ = "none";
    ran_subopt_geo_ = nullptr;
    PlacedChoice choice;
    int gaps = 0;
    const LaunchPlan &plan = subopt_plan_for(alg, mask, choice, gaps);
    hip_check(hipSetDevice(device_), "hipSetDevice");
    const long long chunk = subopt_chunk_pairs(plan, n);
    ensure_subopt_scratch(kSlots, plan, chunk, stream);
    const int track = choice.route == PlacedRoute::Key ? kPlacedKey : kPlacedRows;
    for (long long begin = 0; begin < n; begin += chunk)           // (stream order: the next chunk reuses the scratch behind this one's records)
        subopt_chunk(kSlots, plan, track, gaps, std::min(chunk, n - begin), d_reads + (size_t)begin * R_, d_refs + (size_t)begin * F_, mask, d_subopt + begin, stream);
    ran_subopt_ = ran_placed_name(choice.route);
    subopt_ring_cols_ = subopt_ring_cols(plan.geo->G);
}

// Host pointers in, host records out: record_pipeline, each slot with a scratch of its own (a quarter of the device call's),
// a slot's chunk cut to it in stream order, 20 bytes per pair on the way back.
void Engine::score_subopt_host(int opt, int n, const char *const *reads, const char *const *refs, int mask, SuboptRec *subopt, int threads) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ran_subopt_ = "none";
    ran_subopt_geo_ = nullptr;
    PlacedChoice choice;
    int gaps = 0;
    const LaunchPlan &plan = subopt_plan_for(alg, mask, choice, gaps);          // (refusals leave here, before anything is staged)
    const int track = choice.route == PlacedRoute::Key ? kPlacedKey : kPlacedRows;
    const long long chunk = host_chunk_pairs(false, n);
    const long long part = std::max<long long>(plan.pairs_per_wave, subopt_chunk_pairs(plan, chunk) / kSlots / plan.pairs_per_wave * plan.pairs_per_wave);
    reset_pipeline();               // (before a scratch regrows: no chunk of a call that threw still runs)
    for (int s = 0; s < kSlots; ++s) ensure_subopt_scratch(s, plan, std::min(part, chunk), streams_[s].get());
    record_pipeline(n, reads, refs, subopt, RecordKind{sizeof(SuboptRec), "suboptimal records", "D2H suboptimal records"}, chunk, false, threads,
                    [&](int slot, long long cnt, const uint8_t *d_reads, const uint8_t *d_refs, uint8_t *d_records, hipStream_t stream) {
                        for (long long begin = 0; begin < cnt; begin += part)
                            subopt_chunk(slot, plan, track, gaps, std::min(part, cnt - begin), d_reads + (size_t)begin * R_, d_refs + (size_t)begin * F_, mask,
                                         (SuboptRec *)d_records + begin, stream);
                    });
    ran_subopt_ = ran_placed_name(choice.route);
    subopt_ring_cols_ = subopt_ring_cols(plan.geo->G);
}

}  // namespace valign
