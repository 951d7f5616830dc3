// engine_span_cigar.hip -- Engine: spanned CIGARs (include/valign_hip.h: valign_hip_align_span_*): the alignment of every pair's
// span, filled and walked on the span's window read[0, read_end) x ref[ref_end - span_ref_length, ref_end) instead of the whole
// R x F matrix.  span_cigar_choice (cell_rules.h) decides what is refused; this unit launches, per chunk and all on one stream:
// score_placed_device as it stands, span_reverse_kernel (engine_span.hip), align_device of the spanned scores' child engine over
// the reversed prefixes into an engine-owned rows scratch, and span_cigar_encode_kernel (span_cigar_kernels.hip.h) behind the
// child's walk -- launch_cigar of the child, the single hook behind every walk, hands the rows to it.  The rows never cross PCIe.
// The host entry delivers through the packed path of engine_cigar.hip with that encoder, launched through the child, as its emit pass.
#include "engine.hip.h"

namespace valign {

Engine &Engine::span_cigar_prepare(int alg) {
    const LaunchPlan &base = align_base_plan();
    RuleInputs in = rule_inputs();
    in.no_f16 = true;                   // (as span_prepare: placed scores run on int16 cells)
    const PlacedFacts facts = placed_facts();
    const PlacedChoice early = span_choice(in, alg, facts, base.geo->G, base.geo->K);       // (no child engine for a call that is refused anyway)
    if (early.route == PlacedRoute::Refused) throw std::runtime_error(early.reason);
    if (!span_child_) span_child_ = std::make_unique<Engine>(device_, R_, (int)span_ref_length(in), sc_, force_g_, force_k_);
    Engine &child = *span_child_;
    child.set_score_width(score_width_);
    child.set_placed_wide(placed_wide());
    child.scratch_cap_mb_ = scratch_cap_mb_;            // (the key cannot be taken back: the field, not the setter)
    child.trace_checkpoints_ = trace_checkpoints_;
    const SpanCigarChoice choice = span_cigar_choice(in, alg, facts, child.rule_inputs(), child.route_facts(false), base.geo->G, base.geo->K);
    if (choice.refused()) throw std::runtime_error(choice.reason);
    PlacedChoice fwd;
    int gaps = 0;
    (void)placed_plan_for(alg, fwd, gaps);              // (what the forward sweep still refuses leaves here, before anything runs)
    return child;
}

// Pairs of one chunk: what span_cigar_bytes_ holds of reversed prefixes, forward records and the child's rows / idx, in whole
// rounds of the forward sweep's waves; never fewer than 16
long long Engine::span_cigar_chunk_pairs(long long n) const {
    const size_t AL = (size_t)R_ + (size_t)span_child_->ref_length();
    const size_t per_pair = AL + sizeof(PlacedRec) + 2 * AL + 8;
    long long chunk = whole_rounds((long long)(span_cigar_bytes_ / per_pair));
    chunk = std::max<long long>(chunk & ~1ll, 16);
    return std::min(chunk, n);
}

void Engine::ensure_span_cigar_scratch(int c, long long pairs, bool host, hipStream_t stream) {
    SpanCigarCtx &x = span_cigar_[c];
    if (pairs > x.cap) {
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");          // nothing may still use the old scratch
        if (span_child_->trace_stream_) hip_check(hipStreamSynchronize(span_child_->trace_stream_.get()), "hipStreamSynchronize");
        x.cap = 0;
        for (DeviceBuffer<uint8_t> *b : {&x.rev_reads, &x.rev_refs, &x.rows}) b->reset();
        x.fwd.reset();
        x.idx.reset();
        const size_t Fr = (size_t)span_child_->ref_length(), AL = (size_t)R_ + Fr;
        x.rev_reads.reserve(std::max<size_t>((size_t)pairs * R_, 16), "reversed reads");
        x.rev_refs.reserve(std::max<size_t>((size_t)pairs * Fr, 16), "reversed references");
        x.fwd.reserve(sizeof(PlacedRec) * (size_t)pairs, "forward records");
        x.rows.reserve((size_t)pairs * 2 * AL + 64, "alignment rows (spanned CIGARs)");
        x.idx.reserve(sizeof(short) * 4 * (size_t)pairs, "alignment coordinates (spanned CIGARs)");
        x.cap = pairs;
    }
    if (host) {                             // (the host path waits for every chunk: nothing uses these between two calls)
        x.pack.recs.reserve(sizeof(CigarRec) * (size_t)x.cap, "alignment records");
        x.pack.offsets.reserve(sizeof(long long) * ((size_t)x.cap + 1), "op offsets");
        x.h_total.reserve(sizeof(long long), "op total");
    }
}

void Engine::launch_span_cigar_args(hipStream_t stream, SpanCigarArgs &a) {
    a.AL = R_ + F_;                     // (this is the child: F_ is span_ref_length)
    a.R = R_;
    // (the lane group is taken for the shape that is walked; the parent reports it: span_cigar_chunk)
    launch_encoder(stream, a, span_cigar_encode_kernel<16>, span_cigar_encode_kernel<64>, "hipLaunchKernel(span_cigar_encode_kernel)");
}

void Engine::launch_span_cigar(hipStream_t stream, const uint8_t *rows, const short *idx, long long begin, long long cnt) {
    SpanCigarArgs a{};
    a.rows = rows;
    a.idx = idx;
    a.fwd = cigar_->fwd + begin;
    a.recs = cigar_->recs + begin;
    a.ops = cigar_->ops ? cigar_->ops + (size_t)begin * cigar_->ops_stride : nullptr;
    a.ops_stride = cigar_->ops_stride;
    a.n = cnt;
    a.F = cigar_->fwd_ref_length;
    a.extended = cigar_->extended;
    launch_span_cigar_args(stream, a);
}

void Engine::span_cigar_chunk(int c, int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, const CigarSink &sink, hipStream_t stream) {
    SpanCigarCtx &x = span_cigar_[c];
    Engine &child = *span_child_;
    if (n > x.cap) throw std::runtime_error("spanned CIGARs: chunk larger than its scratch");
    score_placed_device(opt, n, d_reads, d_refs, x.fwd.get(), stream);
    launch_span_reverse(n, d_reads, d_refs, x.fwd.get(), x.rev_reads.get(), x.rev_refs.get(), child.ref_length(), stream);
    child.ran_cigar_lanes_ = 0;
    {
        ScopedSink scoped(child.cigar_, &sink);
        (void)child.align_device(opt, n, x.rev_reads.get(), x.rev_refs.get(), x.rows.get(), x.idx.get(), stream);
    }
    ran_cigar_lanes_ = child.ran_cigar_lanes_;          // the width the child's encoder ran on
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ran_span_cigar_ = std::string(ran_placed_) + "/" + child.ran_align_fill();
}

void Engine::align_span_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int extended, CigarRec *d_recs, unsigned *d_ops,
                               int ops_stride, hipStream_t stream) {
    ran_span_cigar_ = "none";
    ran_cigar_lanes_ = 0;
    check_packed_device_args(extended, ops_stride, d_recs, d_ops);
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;          // reference: unsupported mode is a silent no-op
    ran_placed_ = ran_placed_name(PlacedRoute::Refused);
    ran_placed_geo_ = nullptr;
    ran_result_format_ = "cigar";
    (void)span_cigar_prepare(alg);          // (refusals leave here, before anything is launched)
    hip_check(hipSetDevice(device_), "hipSetDevice");
    const long long chunk = span_cigar_chunk_pairs(n);
    ensure_span_cigar_scratch(1, chunk, false, stream);
    for (long long begin = 0; begin < n; begin += chunk) {         // (stream order: the next chunk reuses the scratch behind this one's encoder)
        CigarSink sink{d_recs + begin, d_ops + (size_t)begin * ops_stride, ops_stride, extended};
        sink.fwd = span_cigar_[1].fwd.get();
        sink.fwd_ref_length = F_;
        span_cigar_chunk(1, opt, std::min(chunk, n - begin), d_reads + (size_t)begin * R_, d_refs + (size_t)begin * F_, sink, stream);
    }
}

// Host pointers in, packed results out.  Chunk after chunk on streams_[0], each waited for: the raw staging, the chunk above with
// a records-only sink (count pass), then the packed delivery of engine_cigar.hip -- scan, op total, emit pass at the scanned
// offsets beside the records, ONE copy back, unpacking -- with the child's backward encoder as the emit pass.  Chunks do not
// overlap (the fill of the window is short beside the forward sweep, and the pipeline of align_cigar_host can be put
// under this loop when a profile asks for it).
bool Engine::align_span_host(int opt, int n, const char *const *reads, const char *const *refs, int extended, CigarRec *recs, unsigned *ops,
                             long long ops_cap, long long *offsets, long long *ops_needed, int threads) {
    ran_span_cigar_ = "none";
    ran_cigar_lanes_ = 0;
    check_packed_host_args(extended, n, recs, ops, ops_cap, offsets, ops_needed);
    const int alg = opt & 0xF;
    if (alg > 1) return true;                       // (the same silent no-op as every entry point)
    offsets[0] = 0;
    *ops_needed = 0;
    cigar_d2h_bytes_ = 0;
    if (n == 0) return true;
    if (!reads || !refs) throw std::runtime_error("null sequence array");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ran_placed_ = ran_placed_name(PlacedRoute::Refused);
    ran_placed_geo_ = nullptr;
    ran_result_format_ = "cigar";
    Engine &child = span_cigar_prepare(alg);        // (refusals leave here, before anything is staged)
    hip_check(hipSetDevice(device_), "hipSetDevice");
    // (the chunks of align_cigar_host, inside the spanned scratch's bound)
    const long long chunk = std::min<long long>(packed_chunk_pairs(align_chunk_bytes_), span_cigar_chunk_pairs(n));
    reset_pipeline();
    ensure_staging(chunk);
    threads = std::min(std::max(threads, 1), 64);
    hipStream_t st = streams_[0].get();
    ensure_span_cigar_scratch(0, chunk, true, st);
    SpanCigarCtx &x = span_cigar_[0];
    host_stats_ = HostStats{};
    struct Quiesce {            // an error part-way leaves nothing in flight
        Engine *child;
        hipStream_t st;
        bool armed = true;
        ~Quiesce() {
            child->cigar_ = nullptr;
            if (!armed) return;
            if (child->trace_stream_) (void)hipStreamSynchronize(child->trace_stream_.get());
            (void)hipStreamSynchronize(st);
        }
    } quiesce{&child, st};
    auto wait = [&] {
        auto t0 = std::chrono::steady_clock::now();
        hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
        host_stats_.wait_ms += ms_between(t0, std::chrono::steady_clock::now());
    };
    OpsBudget budget{ops_cap};
    for (long long begin = 0; begin < n; begin += chunk) {
        const long long cnt = std::min<long long>(chunk, n - begin);
        stage_raw_chunk(0, st, reads + begin, refs + begin, cnt, threads);
        CigarSink sink{x.pack.recs.get(), nullptr, 1, extended};        // records only: the ops wait for the chunk's scan
        sink.fwd = x.fwd.get();
        sink.fwd_ref_length = F_;
        span_cigar_chunk(0, opt, cnt, d_reads_[0].get(), d_refs_[0].get(), sink, st);
        finish_count_pass(x.pack, cnt, x.h_total.get(), st);
        wait();
        const long long total = x.h_total.get()[0];
        const PackedLayout layout(cnt, 0, total, budget.add(total));
        emit_packed(x.pack, layout, [&](unsigned *d_ops, CigarRec *recs_out) {
            SpanCigarArgs a = emit_args<SpanCigarArgs>(x.pack, x.rows.get(), x.idx.get(), cnt, extended, d_ops, recs_out);
            a.fwd = x.fwd.get();
            a.F = F_;                               // (the parent's: AL and R are the child's)
            child.launch_span_cigar_args(st, a);
            hip_check(hipSetDevice(device_), "hipSetDevice");
        }, nullptr, st);
        wait();
        drain_packed(x.pack, layout, begin, recs, nullptr, ops, offsets, threads);
    }
    quiesce.armed = false;
    *ops_needed = budget.total;
    return budget.fits();
}

}  // namespace valign
