// engine_placed.hip -- Engine: placed Smith-Waterman scores (include/valign_hip.h: valign_hip_score_placed_*): score and end
// cell of every pair from the score sweep alone.  placed_choice (cell_rules.h) decides what a call is -- refused, the register
// sweep with the lane key or the per-row arg-max (placed_kernels.hip.h), the row strips (engine_align.hip), the banded chain
// (engine_long.hip) or, under placed_wide = 1, the int32 sweep (placed_wide_kernels.hip.h) -- and this unit launches it.
// score_placed_strips is the one pointer-free strip sweep, of the int16 strips and the int32 sweeps alike (extension scores under
// extend_wide = 1 run on it too: engine_extend.hip); the host-pointer path is record_pipeline (engine_score.hip) with 12-byte
// records on the way back.
// placed_records_kernel and placed_wide_records_kernel (not templates) are defined in this translation unit.
#define VALIGN_TU_PLACED 1
#include "engine.hip.h"
#include "placed_wide_kernels.hip.h"

namespace valign {

PlacedFacts Engine::placed_facts() const {
    return PlacedFacts{band_width_, score_width_, force_g_ != 0 || force_k_ != 0, align_base_plan().long_mode, band_placed_, band_plan_.usable && !no_band_chain_, placed_wide_,
                       extend_wide_, extend_band_, extend_band_align_};
}

// The plan a placed call runs on: the one alignments start from where its geometry carries the kernel the rule asks for;
// otherwise the cheapest full geometry that fits the read (kernel_instances.hip.h), where the rule is asked again -- the
// key's bits follow the rows per lane.  Throws what the rule refuses.
const LaunchPlan &Engine::placed_plan_for(int alg, PlacedChoice &choice, int &gaps) {
    const LaunchPlan &base = align_base_plan();
    const PlacedFacts facts = placed_facts();
    RuleInputs in = rule_inputs();
    in.no_f16 = true;                   // placed scores run on int16 cells: the gap form is one of the four integer ones
    choice = placed_choice(in, alg, facts, base.geo->G, base.geo->K);
    if (choice.route == PlacedRoute::Refused) throw std::runtime_error(choice.reason);
    gaps = score_gap_form(in, kAlgSW, R_, F_, base.geo->G * base.geo->K);
    if (choice.route == PlacedRoute::Strip || choice.route == PlacedRoute::Chain || choice.route == PlacedRoute::Wide) return base;      // (none launches on the plan)
    auto track_of = [](const PlacedChoice &c) { return c.route == PlacedRoute::Key ? kPlacedKey : kPlacedRows; };
    if (base.geo->placed(track_of(choice), gaps)) return base;
    if (!fallback_plan_.geo) fallback_plan_ = choose_plan(R_, F_, 0, 0, false, true);
    choice = placed_choice(in, alg, facts, fallback_plan_.geo->G, fallback_plan_.geo->K);
    if (fallback_plan_.long_mode || !fallback_plan_.geo->placed(track_of(choice), gaps)) throw std::runtime_error("no placed-score kernel for this mode");
    return fallback_plan_;
}

void Engine::score_placed_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, PlacedRec *d_placed, hipStream_t stream) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;          // reference: unsupported mode is a silent no-op
    ran_placed_ = ran_placed_name(PlacedRoute::Refused);
    ran_placed_geo_ = nullptr;
    PlacedChoice choice;
    int gaps = 0;
    const LaunchPlan &plan = placed_plan_for(alg, choice, gaps);
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (choice.route == PlacedRoute::Strip || choice.route == PlacedRoute::Wide) {
        score_placed_strips(choice.route == PlacedRoute::Strip ? placed_strip_sweep(d_placed) : placed_wide_sweep(d_placed), n, d_reads, d_refs, stream);
    } else if (choice.route == PlacedRoute::Chain) {
        // the banded score sweep's launch (engine_long.hip) with the kernel's PLACED form: int32 cells, nothing kept in HBM
        sync_band_tables(stream);
        score_band_device(long_mode(kAlgSW, false), n, d_reads, d_refs, nullptr, d_placed, stream);
    } else {
        PlacedArgs a{};
        a.reads = d_reads;
        a.refs = d_refs;
        a.placed = d_placed;
        a.n = n;
        a.R = R_;
        a.F = F_;
        put_lds(a, plan.lds);
        put_scoring(a);
        const void *fn = plan.geo->placed(choice.route == PlacedRoute::Key ? kPlacedKey : kPlacedRows, gaps);
        ran_placed_geo_ = plan.geo;
        const long long ppb = (long long)plan.pairs_per_wave * plan.waves_per_block;
        const long long blocks = (n + ppb - 1) / ppb;
        if (blocks > 0x7FFFFFFFll) throw std::runtime_error("batch too large for one launch");
        const int block_lds = plan.lds.total * plan.waves_per_block;
        raise_block_lds(fn, block_lds);
        void *kargs[] = {&a};
        hip_check(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(plan.waves_per_block * kWave), kargs, (size_t)block_lds, stream),
                  "hipLaunchKernel(score_placed_kernel)");
    }
    ran_placed_ = ran_placed_name(choice.route);
}

// placed_wide = 1: the int32 sweep.  8 rows per lane, the K of the int32 Smith-Waterman alignment strips; a row set is one int32
// row per pair (and an F row beside it, affine); no first-invalid table.
Engine::PlacedSweep Engine::placed_wide_sweep(PlacedRec *d_placed) const {
    constexpr int K = 8;
    const void *fn = sc_.affine ? (const void *)&score_placed_wide_kernel<K, true> : (const void *)&score_placed_wide_kernel<K, false>;
    return PlacedSweep{fn, WaveLds{StripLds<K>::kRing, 0, StripLds<K>::kTotal}, strip_plan(R_, F_, K, StripMode{kAlgSW, sc_.affine, false, true, false, false}, kNoBand),
                       false, "placed-score boundary rows (int32)", "hipLaunchKernel(score_placed_wide_kernel)", placed_records_step(d_placed, true)};
}

// One record per merged end cell of the chunk
Engine::PlacedSweep::ChunkStep Engine::placed_records_step(PlacedRec *d_placed, bool wide) const {
    return [d_placed, wide](const StripArgs &a, long long begin, hipStream_t stream) {
        auto *records = wide ? &placed_wide_records_kernel : &placed_records_kernel;
        hipLaunchKernelGGL(records, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, (const EndCell *)a.ends, d_placed + begin, a.n);
        hip_check(hipGetLastError(), wide ? "hipLaunchKernel(placed_wide_records_kernel)" : "hipLaunchKernel(placed_records_kernel)");
    };
}

// The strips' sweep without a pointer stream, the per-pair scratch (placed scores: the Smith-Waterman end cell) merged strip after
// strip, earlier strips winning ties.  Nobody walks back, so per pair-of-pairs two row sets that ping-pong are all the scratch
// there is, row_sets rows of row_dwords dwords each: (2 or 4) x row_dwords dwords on int16 cells, twice that on int32 cells.  A
// slot holds the set of every wave, one row after the other: the F rows lie a row of every wave behind the H rows (the kernels'
// set stride, linear gaps too).
void Engine::score_placed_strips(const PlacedSweep &sweep, long long n, const uint8_t *d_reads, const uint8_t *d_refs, hipStream_t stream) {
    const StripPlan &plan = sweep.plan;
    const size_t bytes_per_pp = (size_t)2 * plan.row_sets * plan.row_dwords * 4;
    size_t free_b = 0, total_b = 0;
    hip_check(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
    const long long chunk = strip_chunk_pairs(strip_scratch_cap(free_b + d_placed_rows_.bytes(), scratch_cap_mb_), bytes_per_pp, n);
    const long long waves = chunk / 2;
    const size_t bad_bytes = sweep.first_bad ? sizeof(int) * 2 * (size_t)chunk : 0;
    if ((size_t)waves * bytes_per_pp > d_placed_rows_.bytes() || sweep.pair_bytes * (size_t)chunk > d_placed_ends_.bytes() || bad_bytes > d_placed_bad_.bytes()) {
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");          // nothing may still read the old scratch
        d_placed_rows_.reserve((size_t)waves * bytes_per_pp, sweep.rows_label);
        d_placed_ends_.reserve(sweep.pair_bytes * (size_t)chunk, "placed-score end cells");
        if (sweep.first_bad) {
            d_placed_bad_.reserve(bad_bytes, "placed-score first invalid positions");
            hip_check(hipMemsetAsync(d_placed_bad_.get(), 0, bad_bytes, stream), "hipMemsetAsync");     // (read by the NW variant only)
        }
    }
    raise_block_lds(sweep.fn, sweep.lds.total);
    const size_t f_rows = plan.f_rows_at(waves), slot_dwords = plan.row_sets * f_rows;
    for (long long begin = 0; begin < n; begin += chunk) {
        const long long cnt = std::min(chunk, n - begin), cnt_waves = (cnt + 1) / 2;
        for (int s = 0; s < plan.strips; ++s) {
            StripArgs a = strip_args(d_reads + (size_t)begin * R_, d_refs + (size_t)begin * F_, cnt, plan, sweep.lds, s, d_placed_rows_.get(),
                                     (size_t)((s + 1) & 1) * slot_dwords, (size_t)(s & 1) * slot_dwords, f_rows, d_placed_ends_.get(),
                                     sweep.first_bad ? d_placed_bad_.get() : nullptr);
            if (sweep.bind) sweep.bind(a, chunk);
            if (s == 0 && sweep.open) sweep.open(a, begin, stream);
            void *kargs[] = {&a};
            hip_check(hipLaunchKernel(sweep.fn, dim3((unsigned)cnt_waves), dim3(kWave), kargs, (size_t)sweep.lds.total, stream), sweep.what);
            if (s + 1 == plan.strips) sweep.close(a, begin, stream);
        }
    }
}

// Host pointers in, host records out: record_pipeline, 12 bytes per pair on the way back.
void Engine::score_placed_host(int opt, int n, const char *const *reads, const char *const *refs, PlacedRec *placed, int threads) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ran_placed_ = ran_placed_name(PlacedRoute::Refused);
    ran_placed_geo_ = nullptr;
    PlacedChoice choice;
    int gaps = 0;
    (void)placed_plan_for(alg, choice, gaps);          // (refusals leave here, before anything is staged)
    // (the chain keeps nothing between launches: its chunks run on the slots' own streams; its tables go up once, here)
    if (choice.route == PlacedRoute::Chain) sync_band_tables(streams_[0].get());
    const bool strips = choice.route == PlacedRoute::Strip || choice.route == PlacedRoute::Wide;      // their launches share the boundary rows: one stream, large chunks
    record_pipeline(n, reads, refs, placed, RecordKind{sizeof(PlacedRec), "placed records", "D2H placed records"}, host_chunk_pairs(strips, n), strips, threads,
                    [&](int, long long cnt, const uint8_t *d_reads, const uint8_t *d_refs, uint8_t *d_records, hipStream_t stream) {
                        score_placed_device(opt, cnt, d_reads, d_refs, (PlacedRec *)d_records, stream);
                    });
}

}  // namespace valign
