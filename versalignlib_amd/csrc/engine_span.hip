// engine_span.hip -- Engine: spanned Smith-Waterman scores (include/valign_hip.h: valign_hip_score_span_*): score, end cell and
// BEGIN cell of every pair from two score sweeps -- no pointer stream, no walk, no host round trip.  span_choice (cell_rules.h)
// decides what is refused and span_ref_length how many reference columns the reverse sweep looks back; this unit launches:
// score_placed_device as it stands, span_reverse_kernel, score_placed_device of a child engine of the reverse sweep's shape,
// span_records_kernel.  The host-pointer path is record_pipeline (engine_score.hip) with 20-byte records on the way back.
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

void Engine::launch_span_reverse(long long n, const uint8_t *d_reads, const uint8_t *d_refs, const PlacedRec *fwd, uint8_t *rev_reads, uint8_t *rev_refs,
                                 int Fr, hipStream_t stream) {
    SpanReverseArgs a{};
    a.reads = d_reads;
    a.refs = d_refs;
    a.fwd = fwd;
    a.rev_reads = rev_reads;
    a.rev_refs = rev_refs;
    a.n = n;
    a.R = R_;
    a.F = F_;
    a.Fr = Fr;
    // about 4 KB of destination bytes per block, whole pairs
    a.pairs_per_block = (int)std::min<long long>(64, std::max<long long>(1, 4096 / std::max(1, R_ + a.Fr)));
    const long long blocks = (n + a.pairs_per_block - 1) / a.pairs_per_block;
    if (blocks > 0x7FFFFFFFll) throw std::runtime_error("batch too large for one launch");
    hipLaunchKernelGGL(span_reverse_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    hip_check(hipGetLastError(), "hipLaunchKernel(span_reverse_kernel)");
}

void Engine::span_chunk(int c, int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, SpanRec *d_spans, hipStream_t stream) {
    SpanCtx &x = span_[c];
    Engine &child = *span_child_;
    if (n > x.cap) throw std::runtime_error("spanned scores: chunk larger than its scratch");
    score_placed_device(opt, n, d_reads, d_refs, x.fwd.get(), stream);
    launch_span_reverse(n, d_reads, d_refs, x.fwd.get(), x.rev_reads.get(), x.rev_refs.get(), child.ref_length(), stream);
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
    ran_placed_geo_ = nullptr;
    bool strips = false;
    (void)span_prepare(alg, strips);
    hip_check(hipSetDevice(device_), "hipSetDevice");
    const long long chunk = span_chunk_pairs(n);
    ensure_span_scratch(kSlots, chunk, stream);
    for (long long begin = 0; begin < n; begin += chunk)           // (stream order: the next chunk reuses the scratch behind this one's records)
        span_chunk(kSlots, opt, std::min(chunk, n - begin), d_reads + (size_t)begin * R_, d_refs + (size_t)begin * F_, d_spans + begin, stream);
}

// Host pointers in, host records out: record_pipeline, each slot with a reversal scratch of its own, the four launches of a
// chunk on the chunk's stream, 20 bytes per pair on the way back.
void Engine::score_span_host(int opt, int n, const char *const *reads, const char *const *refs, SpanRec *spans, int threads) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ran_span_ = "none";
    ran_placed_ = ran_placed_name(PlacedRoute::Refused);
    ran_placed_geo_ = nullptr;
    bool strips = false;                                        // their launches share the boundary rows: one stream, large chunks
    (void)span_prepare(alg, strips);                            // (refusals leave here, before anything is staged)
    hip_check(hipSetDevice(device_), "hipSetDevice");
    const long long chunk = host_chunk_pairs(strips, n);
    reset_pipeline();               // (before a scratch regrows: no chunk of a call that threw still runs; record_pipeline's own reset then finds nothing)
    for (int s = 0; s < kSlots; ++s) ensure_span_scratch(s, chunk, streams_[s].get());
    record_pipeline(n, reads, refs, spans, RecordKind{sizeof(SpanRec), "spanned records", "D2H spanned records"}, chunk, strips, threads,
                    [&](int slot, long long cnt, const uint8_t *d_reads, const uint8_t *d_refs, uint8_t *d_records, hipStream_t stream) {
                        span_chunk(slot, opt, cnt, d_reads, d_refs, (SpanRec *)d_records, stream);
                    });
}

}  // namespace valign
