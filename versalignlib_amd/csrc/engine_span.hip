// engine_span.hip -- Engine: spanned Smith-Waterman scores (include/valign_hip.h: valign_hip_score_span_*): score, end cell and
// BEGIN cell of every pair from two score sweeps -- no pointer stream, no walk, no host round trip.  span_choice (cell_rules.h)
// decides what is refused and span_ref_length how many reference columns the reverse sweep looks back; this unit launches:
// score_placed_device as it stands, span_reverse_kernel, score_placed_device of a child engine of the reverse sweep's shape,
// span_records_kernel.  The host-pointer path is score_placed_host's chunk pipeline with 20-byte records on the way back.
// span_reverse_kernel and span_records_kernel (not templates) are defined in this translation unit.
#define VALIGN_TU_SPAN 1
#include "engine.hip.h"

namespace valign {

Engine &Engine::span_prepare(int alg, bool &strips) {
    const LaunchPlan &base = align_base_plan();
    RuleInputs in = rule_inputs();
    in.no_f16 = true;                   // (as placed_plan_for: placed scores run on int16 cells)
    const PlacedChoice refusal = span_choice(in, alg, placed_facts(), base.geo->G, base.geo->K);
    if (refusal.route == PlacedRoute::Refused) throw std::runtime_error(refusal.reason);
    if (!span_child_) span_child_ = std::make_unique<Engine>(device_, R_, (int)span_ref_length(in), sc_, force_g_, force_k_);
    span_child_->set_score_width(score_width_);
    span_child_->set_placed_wide(placed_wide());
    PlacedChoice fwd, rev;
    int gaps = 0;
    (void)placed_plan_for(alg, fwd, gaps);                      // (what either sweep still refuses leaves here, before anything runs)
    (void)span_child_->placed_plan_for(alg, rev, gaps);         // the reverse sweep's rule is asked for its own shape
    auto shared_rows = [](const PlacedChoice &c) { return c.route == PlacedRoute::Strip || c.route == PlacedRoute::Wide; };
    strips = shared_rows(fwd) || shared_rows(rev);
    return *span_child_;
}

// Pairs of one chunk of a device-resident call: what span_scratch_bytes_ holds of reversed sequences and the two record
// buffers, in whole rounds of the forward sweep's waves
long long Engine::span_chunk_pairs(long long n) const {
    const size_t per_pair = (size_t)R_ + (size_t)span_child_->ref_length() + 2 * sizeof(PlacedRec);
    long long chunk = whole_rounds((long long)(span_scratch_bytes_ / per_pair));
    chunk = std::max<long long>(chunk & ~1ll, 16);
    return std::min(chunk, n);
}

void Engine::ensure_span_scratch(int c, long long pairs, hipStream_t stream) {
    SpanCtx &x = span_[c];
    if (pairs <= x.cap) return;
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");          // nothing may still read the old scratch
    x.cap = 0;
    x.rev_reads.reset();
    x.rev_refs.reset();
    x.fwd.reset();
    x.rev.reset();
    x.rev_reads.reserve(std::max<size_t>((size_t)pairs * R_, 16), "reversed reads");
    x.rev_refs.reserve(std::max<size_t>((size_t)pairs * span_child_->ref_length(), 16), "reversed references");
    x.fwd.reserve(sizeof(PlacedRec) * (size_t)pairs, "forward records");
    x.rev.reserve(sizeof(PlacedRec) * (size_t)pairs, "reverse records");
    x.cap = pairs;
}

void Engine::span_chunk(int c, int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, SpanRec *d_spans, hipStream_t stream) {
    SpanCtx &x = span_[c];
    Engine &child = *span_child_;
    if (n > x.cap) throw std::runtime_error("spanned scores: chunk larger than its scratch");
    score_placed_device(opt, n, d_reads, d_refs, x.fwd.get(), stream);
    SpanReverseArgs a{};
    a.reads = d_reads;
    a.refs = d_refs;
    a.fwd = x.fwd.get();
    a.rev_reads = x.rev_reads.get();
    a.rev_refs = x.rev_refs.get();
    a.n = n;
    a.R = R_;
    a.F = F_;
    a.Fr = child.ref_length();
    // about 4 KB of destination bytes per block, whole pairs
    a.pairs_per_block = (int)std::min<long long>(64, std::max<long long>(1, 4096 / std::max(1, R_ + a.Fr)));
    const long long blocks = (n + a.pairs_per_block - 1) / a.pairs_per_block;
    if (blocks > 0x7FFFFFFFll) throw std::runtime_error("batch too large for one launch");
    hipLaunchKernelGGL(span_reverse_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    hip_check(hipGetLastError(), "hipLaunchKernel(span_reverse_kernel)");
    child.score_placed_device(opt, n, x.rev_reads.get(), x.rev_refs.get(), x.rev.get(), stream);
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hipLaunchKernelGGL(span_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const PlacedRec *)x.fwd.get(),
                       (const PlacedRec *)x.rev.get(), d_spans, n);
    hip_check(hipGetLastError(), "hipLaunchKernel(span_records_kernel)");
    ran_span_ = std::string(ran_placed_) + "/" + child.ran_placed();
}

void Engine::score_span_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, SpanRec *d_spans, hipStream_t stream) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;          // reference: unsupported mode is a silent no-op
    ran_span_ = "none";
    ran_placed_ = ran_placed_name(PlacedRoute::Refused);
    bool strips = false;
    (void)span_prepare(alg, strips);
    hip_check(hipSetDevice(device_), "hipSetDevice");
    const long long chunk = span_chunk_pairs(n);
    ensure_span_scratch(kSlots, chunk, stream);
    for (long long begin = 0; begin < n; begin += chunk)           // (stream order: the next chunk reuses the scratch behind this one's records)
        span_chunk(kSlots, opt, std::min(chunk, n - begin), d_reads + (size_t)begin * R_, d_refs + (size_t)begin * F_, d_spans + begin, stream);
}

void Engine::ensure_span_staging(long long pairs) {
    if (pairs <= span_staged_pairs_) return;
    span_staged_pairs_ = 0;
    for (int s = 0; s < kSlots; ++s) {
        h_span_[s].reset();
        d_span_[s].reset();
    }
    for (int s = 0; s < kSlots; ++s) {
        h_span_[s].reserve(sizeof(SpanRec) * (size_t)pairs);
        d_span_[s].reserve(sizeof(SpanRec) * (size_t)pairs, "spanned records");
    }
    span_staged_pairs_ = pairs;
}

// Host pointers in, host records out: score_placed_host's pipeline -- gather, pinned staging (4-bit classes where host_packing
// is on), H2D, the four launches of a chunk, D2H -- over kSlots slots, each with a reversal scratch of its own.
void Engine::score_span_host(int opt, int n, const char *const *reads, const char *const *refs, SpanRec *spans, int threads) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ran_span_ = "none";
    ran_placed_ = ran_placed_name(PlacedRoute::Refused);
    bool strips = false;                                        // their launches share the boundary rows: one stream, large chunks
    (void)span_prepare(alg, strips);                            // (refusals leave here, before anything is staged)
    hip_check(hipSetDevice(device_), "hipSetDevice");
    const size_t per_pair = (size_t)R_ + F_;
    const size_t chunk_bytes = strips && !dbg_.on("chunk_bytes") ? std::max<size_t>(score_chunk_bytes_, 192u << 20) : score_chunk_bytes_;
    long long chunk = per_pair ? (long long)(chunk_bytes / per_pair) : n;
    chunk = whole_rounds(chunk);
    chunk = std::max<long long>(chunk, 1024);
    chunk = std::min<long long>(chunk, n);
    reset_pipeline();
    ensure_staging(chunk);
    ensure_span_staging(chunk);
    for (int s = 0; s < kSlots; ++s) ensure_span_scratch(s, chunk, streams_[s].get());
    threads = std::min(std::max(threads, 1), 64);
    host_stats_ = HostStats{};
    if (direct_call(n, per_pair)) {
        // small call: the kernels read the gathered sequences out of the pinned staging and write the records there
        auto t0 = std::chrono::steady_clock::now();
        gather(reads, refs, n, h_reads_[0].get(), h_refs_[0].get(), threads);
        auto t1 = std::chrono::steady_clock::now();
        span_chunk(0, opt, n, dev_view(h_reads_[0].get()), dev_view(h_refs_[0].get()), (SpanRec *)dev_view(h_span_[0].get()), streams_[0].get());
        hip_check(hipStreamSynchronize(streams_[0].get()), "hipStreamSynchronize");
        auto t2 = std::chrono::steady_clock::now();
        memcpy(spans, h_span_[0].get(), sizeof(SpanRec) * (size_t)n);
        host_stats_.gather_ms = ms_between(t0, t1);
        host_stats_.wait_ms = ms_between(t1, t2);
        host_stats_.drain_ms = ms_between(t2, std::chrono::steady_clock::now());
        host_stats_.direct = 1;
        return;
    }
    auto drain = [&](int s) {
        if (slot_pending_[s] <= 0) return;
        memcpy(spans + slot_begin_[s], h_span_[s].get(), sizeof(SpanRec) * (size_t)slot_pending_[s]);
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
        span_chunk(slot, opt, cnt, d_reads, d_refs, d_span_[slot].get(), st);
        hip_check(hipMemcpyAsync(h_span_[slot].get(), d_span_[slot].get(), sizeof(SpanRec) * (size_t)cnt, hipMemcpyDeviceToHost, st), "D2H spanned records");
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
