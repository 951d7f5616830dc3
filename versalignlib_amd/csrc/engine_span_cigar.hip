// engine_span_cigar.hip -- Engine: spanned CIGARs (include/valign_hip.h: valign_hip_align_span_*): the alignment of every pair's
// span, filled and walked on the span's window read[0, read_end) x ref[ref_end - span_ref_length, ref_end) instead of the whole
// R x F matrix.  span_cigar_choice (cell_rules.h) decides what is refused; this unit launches, per chunk and all on one stream:
// score_placed_device as it stands, span_reverse_kernel (engine_span.hip), align_device of the spanned scores' child engine over
// the reversed prefixes into an engine-owned rows scratch, and span_cigar_encode_kernel (span_cigar_kernels.hip.h) behind the
// child's walk -- launch_cigar of the child, the single hook behind every walk, hands the rows to it.  The rows never cross PCIe.
#include "engine.hip.h"

namespace valign {

namespace {
// the child's sink for the time of its alignment call, cleared however the call leaves
template <class T>
struct ScopedSink {
    const T *&slot;
    ScopedSink(const T *&s, const T *value) : slot(s) { slot = value; }
    ~ScopedSink() { slot = nullptr; }
};
}  // namespace

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
        x.recs.reserve(sizeof(CigarRec) * (size_t)x.cap, "alignment records");
        x.offsets.reserve(sizeof(long long) * ((size_t)x.cap + 1), "op offsets");
        x.h_total.reserve(sizeof(long long), "op total");
    }
}

void Engine::launch_span_cigar_args(hipStream_t stream, SpanCigarArgs &a) {
    a.AL = R_ + F_;                     // (this is the child: F_ is span_ref_length)
    a.R = R_;
    a.affine = sc_.affine ? 1 : 0;
    a.match = sc_.match;
    a.mismatch = sc_.mismatch;
    a.gap_read = sc_.gap_read;
    a.gap_ref = sc_.gap_ref;
    a.open_read = sc_.open_read;
    a.ext_read = sc_.ext_read;
    a.open_ref = sc_.open_ref;
    a.ext_ref = sc_.ext_ref;
    const int lanes = take_cigar_lanes();          // for the shape that is walked; the parent reports it (span_cigar_chunk)
    const long long per_block = 256 / lanes;
    const long long blocks = (a.n + per_block - 1) / per_block;
    if (blocks > 0x7FFFFFFFll) throw std::runtime_error("batch too large for one launch");
    const dim3 grid((unsigned)blocks), block(256);
    if (lanes == 16) hipLaunchKernelGGL(span_cigar_encode_kernel<16>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(span_cigar_encode_kernel<64>, grid, block, 0, stream, a);
    hip_check(hipGetLastError(), "hipLaunchKernel(span_cigar_encode_kernel)");
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
        ScopedSink<CigarSink> scoped(child.cigar_, &sink);
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
    if (extended != 0 && extended != 1) throw std::runtime_error("extended must be 0 (M) or 1 (= / X)");
    if (ops_stride < 1) throw std::runtime_error("ops_stride must be >= 1");
    if (!d_recs || !d_ops) throw std::runtime_error("null result buffer");
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

// Host pointers in, packed results out.  Chunk after chunk on streams_[0], each waited for: gather, H2D, the chunk above with a
// records-only sink (count pass), the scan of n_ops, the op total to the host, the emit pass at the scanned offsets beside the
// records, ONE copy of records + ops back.  Chunks do not overlap (the fill of the window is short beside the
// forward sweep, and the pipeline of align_cigar_host can be put under this loop when a profile asks for it).
bool Engine::align_span_host(int opt, int n, const char *const *reads, const char *const *refs, int extended, CigarRec *recs, unsigned *ops,
                             long long ops_cap, long long *offsets, long long *ops_needed, int threads) {
    ran_span_cigar_ = "none";
    ran_cigar_lanes_ = 0;
    if (extended != 0 && extended != 1) throw std::runtime_error("extended must be 0 (M) or 1 (= / X)");
    if (!recs || !offsets || !ops_needed || (!ops && ops_cap > 0)) throw std::runtime_error("null result buffer");
    if (n < 0 || ops_cap < 0) throw std::runtime_error("negative size");
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
    const size_t per_pair = (size_t)3 * (R_ + F_) + 8;         // (the chunks of align_cigar_host, inside the spanned scratch's bound)
    long long chunk = std::max<long long>(whole_rounds((long long)(align_chunk_bytes_ / per_pair)), 1024);
    chunk = std::min<long long>(chunk, span_cigar_chunk_pairs(n));
    reset_pipeline();
    ensure_staging(chunk);
    threads = std::min(std::max(threads, 1), 64);
    hipStream_t st = streams_[0].get();
    ensure_span_cigar_scratch(0, chunk, true, st);
    SpanCigarCtx &x = span_cigar_[0];
    host_stats_ = HostStats{};
    struct Quiesce {            // an error part-way leaves nothing in flight
        Engine *e, *child;
        hipStream_t st;
        bool armed = true;
        ~Quiesce() {
            child->cigar_ = nullptr;
            if (!armed) return;
            if (child->trace_stream_) (void)hipStreamSynchronize(child->trace_stream_.get());
            (void)hipStreamSynchronize(st);
        }
    } quiesce{this, &child, st};
    long long total_ops = 0;
    for (long long begin = 0; begin < n; begin += chunk) {
        const long long cnt = std::min<long long>(chunk, n - begin);
        uint8_t *h_reads = h_reads_[0].get(), *h_refs = h_refs_[0].get(), *d_reads = d_reads_[0].get(), *d_refs = d_refs_[0].get();
        auto t0 = std::chrono::steady_clock::now();
        gather(reads + begin, refs + begin, cnt, h_reads, h_refs, threads);
        host_stats_.gather_ms += ms_between(t0, std::chrono::steady_clock::now());
        hip_check(hipMemcpyAsync(d_reads, h_reads, (size_t)cnt * R_, hipMemcpyHostToDevice, st), "H2D reads");
        hip_check(hipMemcpyAsync(d_refs, h_refs, (size_t)cnt * F_, hipMemcpyHostToDevice, st), "H2D refs");
        CigarSink sink{x.recs.get(), nullptr, 1, extended};        // records only: the ops wait for the chunk's scan
        sink.fwd = x.fwd.get();
        sink.fwd_ref_length = F_;
        span_cigar_chunk(0, opt, cnt, d_reads, d_refs, sink, st);
        launch_cigar_scan(x.recs.get(), x.offsets.get(), cnt, st);
        hip_check(hipMemcpyAsync(x.h_total.get(), x.offsets.get() + cnt, sizeof(long long), hipMemcpyDeviceToHost, st), "D2H op total");
        t0 = std::chrono::steady_clock::now();
        hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
        host_stats_.wait_ms += ms_between(t0, std::chrono::steady_clock::now());
        const long long total = x.h_total.get()[0];
        total_ops += total;
        const bool with_ops = total_ops <= ops_cap;
        const size_t rec_bytes = sizeof(CigarRec) * (size_t)cnt, bytes = rec_bytes + (with_ops ? sizeof(unsigned) * (size_t)total : 0);
        if (bytes > x.h_out.bytes()) {
            x.h_out.reserve(bytes + bytes / 4, "packed alignment results");
            x.out.reserve(bytes + bytes / 4, "packed alignment results");
        }
        const uint8_t *src = reinterpret_cast<const uint8_t *>(x.recs.get());
        if (with_ops) {                             // emit pass: the ops at their offsets, the records beside them
            SpanCigarArgs a{};
            a.rows = x.rows.get();
            a.idx = x.idx.get();
            a.fwd = x.fwd.get();
            a.ops = reinterpret_cast<unsigned *>(x.out.get() + rec_bytes);
            a.offsets = x.offsets.get();
            a.recs_in = x.recs.get();
            a.recs_out = reinterpret_cast<CigarRec *>(x.out.get());
            a.n = cnt;
            a.F = F_;
            a.extended = extended;
            child.launch_span_cigar_args(st, a);
            hip_check(hipSetDevice(device_), "hipSetDevice");
            src = x.out.get();
        }
        hip_check(hipMemcpyAsync(x.h_out.get(), src, bytes, hipMemcpyDeviceToHost, st), "D2H records + ops");
        cigar_d2h_bytes_ += (long long)(bytes + sizeof(long long));
        t0 = std::chrono::steady_clock::now();
        hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
        auto t1 = std::chrono::steady_clock::now();
        const uint8_t *h = x.h_out.get();
        const CigarRec *h_recs = reinterpret_cast<const CigarRec *>(h);
        for_ranges(threads, cnt, 4096, [&](int, long long lo, long long hi) { memcpy(recs + begin + lo, h_recs + lo, sizeof(CigarRec) * (size_t)(hi - lo)); });
        long long at = offsets[begin];
        for (long long i = 0; i < cnt; ++i) {                    // offsets follow from n_ops: rebased on the host
            at += h_recs[i].n_ops;
            offsets[begin + i + 1] = at;
        }
        if (with_ops && total > 0) {
            unsigned *to = ops + offsets[begin];
            const unsigned *from = reinterpret_cast<const unsigned *>(h + rec_bytes);
            for_ranges(threads, total, 1 << 16, [&](int, long long lo, long long hi) { memcpy(to + lo, from + lo, sizeof(unsigned) * (size_t)(hi - lo)); });
        }
        host_stats_.wait_ms += ms_between(t0, t1);
        host_stats_.drain_ms += ms_between(t1, std::chrono::steady_clock::now());
    }
    quiesce.armed = false;
    *ops_needed = total_ops;
    return total_ops <= ops_cap;
}

}  // namespace valign
