// engine_placed.hip -- Engine: placed Smith-Waterman scores (include/valign_hip.h: valign_hip_score_placed_*): score and end
// cell of every pair from the score sweep alone.  placed_choice (cell_rules.h) decides what a call is -- refused, the register
// sweep with the lane key or the per-row arg-max (placed_kernels.hip.h), the row strips (engine_align.hip), the banded chain
// (engine_long.hip) or, under placed_wide = 1, the int32 sweep (placed_wide_kernels.hip.h) -- and this unit launches it; the host-pointer path is score_host's chunk pipeline with 12-byte records on the way back.
// placed_records_kernel and placed_wide_records_kernel (not templates) are defined in this translation unit.
#define VALIGN_TU_PLACED 1
#include "engine.hip.h"
#include "placed_wide_kernels.hip.h"

namespace valign {

PlacedFacts Engine::placed_facts() const {
    return PlacedFacts{band_width_, score_width_, force_g_ != 0 || force_k_ != 0, align_base_plan().long_mode, band_placed_, band_plan_.usable && !no_band_chain_, placed_wide_};
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
    PlacedChoice choice;
    int gaps = 0;
    const LaunchPlan &plan = placed_plan_for(alg, choice, gaps);
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (choice.route == PlacedRoute::Strip) {
        score_placed_strips(n, d_reads, d_refs, d_placed, stream);
        ran_placed_ = ran_placed_name(choice.route);
        return;
    }
    if (choice.route == PlacedRoute::Wide) {
        score_placed_wide(n, d_reads, d_refs, d_placed, stream);
        ran_placed_ = ran_placed_name(choice.route);
        return;
    }
    if (choice.route == PlacedRoute::Chain) {
        // the banded score sweep's launch (engine_long.hip) with the kernel's PLACED form: int32 cells, nothing kept in HBM
        sync_band_tables(stream);
        score_band_device(long_mode(kAlgSW, false), n, d_reads, d_refs, nullptr, d_placed, stream);
        ran_placed_ = ran_placed_name(choice.route);
        return;
    }
    PlacedArgs a{};
    a.reads = d_reads;
    a.refs = d_refs;
    a.placed = d_placed;
    a.n = n;
    a.R = R_;
    a.F = F_;
    a.prof_area = plan.lds.prof_area;
    a.refc_stride = plan.lds.refc_stride;
    a.wave_lds = plan.lds.total;
    put_scoring(a);
    const void *fn = plan.geo->placed(choice.route == PlacedRoute::Key ? kPlacedKey : kPlacedRows, gaps);
    const long long ppb = (long long)plan.pairs_per_wave * plan.waves_per_block;
    const long long blocks = (n + ppb - 1) / ppb;
    if (blocks > 0x7FFFFFFFll) throw std::runtime_error("batch too large for one launch");
    const int block_lds = plan.lds.total * plan.waves_per_block;
    if (block_lds > kDefaultBlockLds)
        hip_check(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, block_lds), "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    void *kargs[] = {&a};
    hip_check(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(plan.waves_per_block * kWave), kargs, (size_t)block_lds, stream),
              "hipLaunchKernel(score_placed_kernel)");
    ran_placed_ = ran_placed_name(choice.route);
}

void Engine::launch_placed_records(const EndCell *d_ends, PlacedRec *d_placed, long long n, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(placed_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_ends, d_placed, n);
    hip_check(hipGetLastError(), "hipLaunchKernel(placed_records_kernel)");
}

// placed_wide = 1: score_placed_strips with the int32 sweep.  8 rows per lane, the K of the int32 Smith-Waterman alignment strips;
// per pair-of-pairs two row sets that ping-pong, each one int32 row per pair (and an F row beside it, affine) -- the wide strip
// plan's row_bytes -- and no pointer region.  The scratch is score_placed_strips' own (a call of the other kind regrows it).
void Engine::score_placed_wide(long long n, const uint8_t *d_reads, const uint8_t *d_refs, PlacedRec *d_placed, hipStream_t stream) {
    constexpr int K = 8;
    const StripMode mode{kAlgSW, sc_.affine, false, true, false, false};
    const StripPlan plan = strip_plan(R_, F_, K, mode, kNoBand);
    const size_t bytes_per_pp = plan.row_bytes;             // 2 slots x row_sets x row_dwords dwords
    size_t free_b = 0, total_b = 0;
    hip_check(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
    const long long chunk = strip_chunk_pairs(strip_scratch_cap(free_b + d_placed_rows_.bytes(), scratch_cap_mb_), bytes_per_pp, n);
    const long long waves = chunk / 2;
    if ((size_t)waves * bytes_per_pp > d_placed_rows_.bytes() || sizeof(EndCell) * (size_t)chunk > d_placed_ends_.bytes()) {
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");          // nothing may still read the old scratch
        d_placed_rows_.reserve((size_t)waves * bytes_per_pp, "placed-score boundary rows (int32)");
        d_placed_ends_.reserve(sizeof(EndCell) * (size_t)chunk, "placed-score end cells");
    }
    const void *fn = sc_.affine ? (const void *)&score_placed_wide_kernel<K, true> : (const void *)&score_placed_wide_kernel<K, false>;
    const WaveLds lds{StripLds<K>::kRing, 0, StripLds<K>::kTotal};
    if (lds.total > kDefaultBlockLds)
        hip_check(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds.total), "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    const size_t set_dwords = (size_t)waves * plan.row_dwords;                    // one row of every wave
    const size_t slot_dwords = (size_t)plan.row_sets * set_dwords;
    for (long long begin = 0; begin < n; begin += chunk) {
        const long long cnt = std::min(chunk, n - begin), cnt_waves = (cnt + 1) / 2;
        for (int s = 0; s < plan.strips; ++s) {
            StripArgs a{};
            put_sweep(a, d_reads + (size_t)begin * R_, d_refs + (size_t)begin * F_, cnt, plan.blocks8, lds);
            a.ends = d_placed_ends_.get();
            a.bottom = d_placed_rows_.get() + (size_t)(s & 1) * slot_dwords;
            a.top = d_placed_rows_.get() + (size_t)((s + 1) & 1) * slot_dwords;
            a.top_f = a.top + set_dwords;           // (the distance is the kernel's set stride, linear gaps too)
            a.bottom_f = a.bottom + set_dwords;
            a.strip = s;
            a.strips = plan.strips;
            a.row_dwords = plan.row_dwords;
            a.band = kNoBand;
            void *kargs[] = {&a};
            hip_check(hipLaunchKernel(fn, dim3((unsigned)cnt_waves), dim3(kWave), kargs, (size_t)lds.total, stream),
                      "hipLaunchKernel(score_placed_wide_kernel)");
        }
        hipLaunchKernelGGL(placed_wide_records_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, stream, (const EndCell *)d_placed_ends_.get(),
                           d_placed + begin, cnt);
        hip_check(hipGetLastError(), "hipLaunchKernel(placed_wide_records_kernel)");
    }
}

void Engine::ensure_placed_staging(long long pairs) {
    if (pairs <= placed_staged_pairs_) return;
    placed_staged_pairs_ = 0;
    for (int s = 0; s < kSlots; ++s) {
        h_placed_[s].reset();
        d_placed_[s].reset();
    }
    for (int s = 0; s < kSlots; ++s) {
        h_placed_[s].reserve(sizeof(PlacedRec) * (size_t)pairs);
        d_placed_[s].reserve(sizeof(PlacedRec) * (size_t)pairs, "placed records");
    }
    placed_staged_pairs_ = pairs;
}

// Host pointers in, host records out: score_host's pipeline -- gather, pinned staging (4-bit classes where host_packing is on:
// only classes matter), H2D, kernel, D2H -- over kSlots slots, 12 bytes per pair on the way back.
void Engine::score_placed_host(int opt, int n, const char *const *reads, const char *const *refs, PlacedRec *placed, int threads) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ran_placed_ = ran_placed_name(PlacedRoute::Refused);
    PlacedChoice choice;
    int gaps = 0;
    (void)placed_plan_for(alg, choice, gaps);          // (refusals leave here, before anything is staged)
    // (the chain keeps nothing between launches: its chunks run on the slots' own streams; its tables go up once, here)
    if (choice.route == PlacedRoute::Chain) sync_band_tables(streams_[0].get());
    const bool strips = choice.route == PlacedRoute::Strip || choice.route == PlacedRoute::Wide;      // their launches share the boundary rows: one stream, large chunks
    const size_t per_pair = (size_t)R_ + F_;
    const size_t chunk_bytes = strips && !dbg_.on("chunk_bytes") ? std::max<size_t>(score_chunk_bytes_, 192u << 20) : score_chunk_bytes_;
    long long chunk = per_pair ? (long long)(chunk_bytes / per_pair) : n;
    chunk = whole_rounds(chunk);
    chunk = std::max<long long>(chunk, 1024);
    chunk = std::min<long long>(chunk, n);
    reset_pipeline();
    ensure_staging(chunk);
    ensure_placed_staging(chunk);
    threads = std::min(std::max(threads, 1), 64);
    host_stats_ = HostStats{};
    if (direct_call(n, per_pair)) {
        // small call: the kernel reads the gathered sequences out of the pinned staging and writes its records there
        auto t0 = std::chrono::steady_clock::now();
        gather(reads, refs, n, h_reads_[0].get(), h_refs_[0].get(), threads);
        auto t1 = std::chrono::steady_clock::now();
        score_placed_device(opt, n, dev_view(h_reads_[0].get()), dev_view(h_refs_[0].get()), (PlacedRec *)dev_view(h_placed_[0].get()), streams_[0].get());
        hip_check(hipStreamSynchronize(streams_[0].get()), "hipStreamSynchronize");
        auto t2 = std::chrono::steady_clock::now();
        memcpy(placed, h_placed_[0].get(), sizeof(PlacedRec) * (size_t)n);
        host_stats_.gather_ms = ms_between(t0, t1);
        host_stats_.wait_ms = ms_between(t1, t2);
        host_stats_.drain_ms = ms_between(t2, std::chrono::steady_clock::now());
        host_stats_.direct = 1;
        return;
    }
    auto drain = [&](int s) {
        if (slot_pending_[s] <= 0) return;
        memcpy(placed + slot_begin_[s], h_placed_[s].get(), sizeof(PlacedRec) * (size_t)slot_pending_[s]);
        slot_pending_[s] = 0;
    };
    int slot = 0;
    for (long long begin = 0; begin < n; begin += chunk, slot = (slot + 1) % kSlots) {
        const long long cnt = std::min<long long>(chunk, n - begin);
        auto t0 = std::chrono::steady_clock::now();
        hip_check(hipEventSynchronize(slot_done_[slot].get()), "hipEventSynchronize");
        auto t1 = std::chrono::steady_clock::now();
        drain(slot);                            // the result of the chunk that used this slot
        auto t2 = std::chrono::steady_clock::now();
        host_stats_.wait_ms += ms_between(t0, t1);
        host_stats_.drain_ms += ms_between(t1, t2);
        hipStream_t st = streams_[strips ? 0 : slot].get();
        uint8_t *h_reads = h_reads_[slot].get(), *h_refs = h_refs_[slot].get(), *d_reads = d_reads_[slot].get(), *d_refs = d_refs_[slot].get();
        if (pack_) {
            const size_t PR = packed_length(R_), PF = packed_length(F_);
            packer_.gather_packed(reads + begin, refs + begin, cnt, h_reads, h_refs, threads);
            host_stats_.gather_ms += ms_between(t2, std::chrono::steady_clock::now());
            hip_check(hipMemcpyAsync(d_pack_reads_[slot].get(), h_reads, (size_t)cnt * PR, hipMemcpyHostToDevice, st), "H2D reads (classes)");
            hip_check(hipMemcpyAsync(d_pack_refs_[slot].get(), h_refs, (size_t)cnt * PF, hipMemcpyHostToDevice, st), "H2D refs (classes)");
            launch_unpack(d_pack_reads_[slot].get(), d_reads, cnt, R_, st);
            launch_unpack(d_pack_refs_[slot].get(), d_refs, cnt, F_, st);
            host_stats_.packed = 1;
        } else {
            gather(reads + begin, refs + begin, cnt, h_reads, h_refs, threads);
            host_stats_.gather_ms += ms_between(t2, std::chrono::steady_clock::now());
            hip_check(hipMemcpyAsync(d_reads, h_reads, (size_t)cnt * R_, hipMemcpyHostToDevice, st), "H2D reads");
            hip_check(hipMemcpyAsync(d_refs, h_refs, (size_t)cnt * F_, hipMemcpyHostToDevice, st), "H2D refs");
        }
        score_placed_device(opt, cnt, d_reads, d_refs, d_placed_[slot].get(), st);
        hip_check(hipMemcpyAsync(h_placed_[slot].get(), d_placed_[slot].get(), sizeof(PlacedRec) * (size_t)cnt, hipMemcpyDeviceToHost, st), "D2H placed records");
        hip_check(hipEventRecord(slot_done_[slot].get(), st), "hipEventRecord");
        slot_begin_[slot] = begin;
        slot_pending_[slot] = cnt;
    }
    for (int k = 0; k < kSlots; ++k) {          // oldest chunk first
        const int s = (slot + k) % kSlots;
        auto t0 = std::chrono::steady_clock::now();
        hip_check(hipEventSynchronize(slot_done_[s].get()), "hipEventSynchronize");
        auto t1 = std::chrono::steady_clock::now();
        drain(s);
        host_stats_.wait_ms += ms_between(t0, t1);
        host_stats_.drain_ms += ms_between(t1, std::chrono::steady_clock::now());
    }
}

}  // namespace valign
