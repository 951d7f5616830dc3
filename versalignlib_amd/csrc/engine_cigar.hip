// engine_cigar.hip -- Engine: the compact result format (include/valign_hip.h: valign_hip_aln records + 32-bit CIGAR ops).
// The alignment paths of engine_align.hip run unchanged into an engine-owned rows scratch; cigar_encode_kernel
// (cigar_kernels.hip.h) reads each part's rows behind its walk.  The rows never cross PCIe.
#define VALIGN_TU_CIGAR 1
#include "engine.hip.h"

namespace valign {

namespace {
// clears Engine::cigar_ when the call leaves, however it leaves
template <class T>
struct ScopedSink {
    const T *&slot;
    ScopedSink(const T *&s, const T *value) : slot(s) { slot = value; }
    ~ScopedSink() { slot = nullptr; }
};
}  // namespace

void Engine::launch_cigar_args(hipStream_t stream, CigarArgs &a) {
    a.AL = R_ + F_;
    a.affine = sc_.affine ? 1 : 0;
    a.match = sc_.match;
    a.mismatch = sc_.mismatch;
    a.gap_read = sc_.gap_read;
    a.gap_ref = sc_.gap_ref;
    a.open_read = sc_.open_read;
    a.ext_read = sc_.ext_read;
    a.open_ref = sc_.open_ref;
    a.ext_ref = sc_.ext_ref;
    const int lanes = take_cigar_lanes();
    const long long per_block = 256 / lanes;
    const dim3 grid((unsigned)((a.n + per_block - 1) / per_block)), block(256);
    if (lanes == 16) hipLaunchKernelGGL(cigar_encode_kernel<16>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(cigar_encode_kernel<64>, grid, block, 0, stream, a);
    hip_check(hipGetLastError(), "hipLaunchKernel(cigar_encode_kernel)");
}

void Engine::launch_cigar(hipStream_t stream, const uint8_t *rows, const short *idx, const EndCell *ends, long long begin, long long cnt) {
    if (!cigar_ || cnt <= 0) return;
    if (cigar_->fwd) {                      // the child engine of a spanned CIGAR call: the backward encoder (engine_span_cigar.hip)
        launch_span_cigar(stream, rows, idx, begin, cnt);
        return;
    }
    CigarArgs a{};
    a.rows = rows;
    a.idx = idx;
    a.ends = ends;
    a.recs = cigar_->recs + begin;
    a.ops = cigar_->ops ? cigar_->ops + (size_t)begin * cigar_->ops_stride : nullptr;
    a.ops_stride = cigar_->ops_stride;
    a.n = cnt;
    a.extended = cigar_->extended;
    launch_cigar_args(stream, a);
}

void Engine::launch_cigar_scan(const CigarRec *recs, long long *offsets, long long n, hipStream_t stream) {
    hipLaunchKernelGGL(cigar_scan_kernel, dim3(1), dim3(1024), 0, stream, recs, offsets, n);
    hip_check(hipGetLastError(), "hipLaunchKernel(cigar_scan_kernel)");
}

void Engine::ensure_cigar_scratch(int slots, long long pairs, hipStream_t stream) {
    const size_t AL = (size_t)R_ + F_;
    for (int s = 0; s < slots; ++s) {
        if (pairs <= cigar_pairs_[s]) continue;
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");       // nothing may still use the old blocks
        if (trace_stream_) hip_check(hipStreamSynchronize(trace_stream_.get()), "hipStreamSynchronize");
        cigar_pairs_[s] = 0;
        d_cig_rows_[s].reserve((size_t)pairs * 2 * AL + 64, "alignment rows (compact results)");
        d_cig_idx_[s].reserve(sizeof(short) * 4 * (size_t)pairs, "alignment coordinates (compact results)");
        d_cig_recs_[s].reserve(sizeof(CigarRec) * (size_t)pairs, "alignment records");
        d_cig_offsets_[s].reserve(sizeof(long long) * ((size_t)pairs + 1), "op offsets");
        cigar_pairs_[s] = pairs;
    }
    h_cig_total_.reserve(sizeof(long long) * 2, "op totals");
}

void Engine::align_cigar_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int extended, CigarRec *d_recs,
                                unsigned *d_ops, int ops_stride, hipStream_t stream) {
    ran_cigar_lanes_ = 0;                   // (a refused call reports no encoder)
    if (extended != 0 && extended != 1) throw std::runtime_error("extended must be 0 (M) or 1 (= / X)");
    if (ops_stride < 1) throw std::runtime_error("ops_stride must be >= 1");
    if (!d_recs || !d_ops) throw std::runtime_error("null result buffer");
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    // the rows scratch is bounded: a call beyond it runs in chunks, each an alignment call of its own on `stream`
    const size_t AL = (size_t)R_ + F_, cap = (size_t)std::max<long long>(1, dbg_.value("cigar_rows_mb", 512)) << 20;
    const long long chunk = std::min<long long>(n, std::max<long long>(2, (long long)(cap / (2 * AL)) & ~1ll));
    ensure_cigar_scratch(1, chunk, stream);
    for (long long begin = 0; begin < n; begin += chunk) {
        const long long cnt = std::min(chunk, n - begin);
        const CigarSink sink{d_recs + begin, d_ops + (size_t)begin * ops_stride, ops_stride, extended};
        ScopedSink<CigarSink> scoped(cigar_, &sink);
        align_device(opt, cnt, d_reads + (size_t)begin * R_, d_refs + (size_t)begin * F_, d_cig_rows_[0].get(), d_cig_idx_[0].get(), stream);
    }
}

bool Engine::align_cigar_host(int opt, int n, const char *const *reads, const char *const *refs, int extended, CigarRec *recs,
                              unsigned *ops, long long ops_cap, long long *offsets, long long *ops_needed, int threads) {
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
    ran_align_fill_ = "none";
    ran_align_geo_ = nullptr;
    ran_result_format_ = "cigar";           // (before the refusals: a refused call must not report the format of an earlier one)
    const int AL = R_ + F_;
    const size_t per_pair = (size_t)3 * AL + 8;                 // (the chunks of align_host: same launches, same rounds)
    const RouteFacts facts = route_facts(true);
    const AlignRoute route = valign::align_route(rule_inputs(), alg, facts);       // (refusals leave here)
    const bool by_strips = strip_chunks(route, facts);
    const size_t chunk_bytes = by_strips && !dbg_.on("align_chunk_bytes") ? std::max<size_t>(align_chunk_bytes_, 384u << 20) : align_chunk_bytes_;
    long long chunk = (long long)(chunk_bytes / per_pair);
    chunk = whole_rounds(chunk);
    chunk = std::max<long long>(chunk, 1024);
    chunk = std::min<long long>(chunk, n);
    reset_pipeline();
    ensure_staging(chunk);
    threads = std::min(std::max(threads, 1), 64);
    hipStream_t kernels = streams_[0].get(), copy_in = streams_[1].get(), copy_out = streams_[2].get();
    ensure_cigar_scratch(2, chunk, kernels);
    host_stats_ = HostStats{};
    const bool small = direct_call(n, (size_t)AL);
    chain_regions_busy_[0] = chain_regions_busy_[1] = false;       // (every earlier call ended with its walks waited for)
    struct Quiesce {            // an error part-way leaves nothing in flight
        Engine *e;
        bool armed = true;
        ~Quiesce() {
            e->cigar_ = nullptr;
            if (!armed) return;
            if (e->trace_stream_) (void)hipStreamSynchronize(e->trace_stream_.get());
            for (int s = 0; s < kSlots; ++s) (void)hipStreamSynchronize(e->streams_[s].get());
        }
    } quiesce{this};
    struct Pending {
        long long begin = 0, cnt = 0, total = 0;
        bool active = false, with_ops = false;
    } pend[2];
    long long total_ops = 0;
    // Chunk in slot s: its records and scanned offsets are on the device and its op total is on its way.  Size the packed
    // output, emit the ops beside the records (copy_out stream: beside the next chunk's fill) and start ONE copy back.
    auto emit = [&](int s) {
        Pending &p = pend[s];
        auto t0 = std::chrono::steady_clock::now();
        hip_check(hipEventSynchronize(kernels_done_[s].get()), "hipEventSynchronize");
        host_stats_.wait_ms += ms_between(t0, std::chrono::steady_clock::now());
        p.total = h_cig_total_.get()[s];
        total_ops += p.total;
        p.with_ops = total_ops <= ops_cap;
        const size_t rec_bytes = sizeof(CigarRec) * (size_t)p.cnt, bytes = rec_bytes + (p.with_ops ? sizeof(unsigned) * (size_t)p.total : 0);
        if (bytes > h_cig_out_[s].bytes()) {                     // (the slot's last copy was drained before the slot was reused)
            h_cig_out_[s].reserve(bytes + bytes / 4, "packed alignment results");
            d_cig_out_[s].reserve(bytes + bytes / 4, "packed alignment results");
        }
        const uint8_t *src = reinterpret_cast<const uint8_t *>(d_cig_recs_[s].get());
        if (p.with_ops) {
            CigarArgs a{};
            a.rows = d_cig_rows_[s].get();
            a.idx = d_cig_idx_[s].get();
            a.ops = reinterpret_cast<unsigned *>(d_cig_out_[s].get() + rec_bytes);
            a.offsets = d_cig_offsets_[s].get();
            a.recs_in = d_cig_recs_[s].get();
            a.recs_out = reinterpret_cast<CigarRec *>(d_cig_out_[s].get());
            a.n = p.cnt;
            a.extended = extended;
            launch_cigar_args(copy_out, a);
            src = d_cig_out_[s].get();
        }
        hip_check(hipMemcpyAsync(h_cig_out_[s].get(), src, bytes, hipMemcpyDeviceToHost, copy_out), "D2H records + ops");
        hip_check(hipEventRecord(slot_done_[s].get(), copy_out), "hipEventRecord");
        cigar_d2h_bytes_ += (long long)(bytes + sizeof(long long));
    };
    auto drain = [&](int s) {
        Pending &p = pend[s];
        if (!p.active) return;
        auto t0 = std::chrono::steady_clock::now();
        hip_check(hipEventSynchronize(slot_done_[s].get()), "hipEventSynchronize");
        auto t1 = std::chrono::steady_clock::now();
        const uint8_t *h = h_cig_out_[s].get();
        const CigarRec *h_recs = reinterpret_cast<const CigarRec *>(h);
        for_ranges(threads, p.cnt, 4096, [&](int, long long lo, long long hi) {
            memcpy(recs + p.begin + lo, h_recs + lo, sizeof(CigarRec) * (size_t)(hi - lo));
        });
        long long at = offsets[p.begin];
        for (long long i = 0; i < p.cnt; ++i) {                  // offsets follow from n_ops: rebased on the host
            at += h_recs[i].n_ops;
            offsets[p.begin + i + 1] = at;
        }
        if (p.with_ops && p.total > 0) {
            unsigned *to = ops + offsets[p.begin];
            const unsigned *from = reinterpret_cast<const unsigned *>(h + sizeof(CigarRec) * (size_t)p.cnt);
            for_ranges(threads, p.total, 1 << 16, [&](int, long long lo, long long hi) { memcpy(to + lo, from + lo, sizeof(unsigned) * (size_t)(hi - lo)); });
        }
        host_stats_.wait_ms += ms_between(t0, t1);
        host_stats_.drain_ms += ms_between(t1, std::chrono::steady_clock::now());
        p.active = false;
    };
    long long chunk_no = 0;
    for (long long begin = 0; begin < n; begin += chunk, ++chunk_no) {
        const int s = (int)(chunk_no & 1);
        const long long cnt = std::min<long long>(chunk, n - begin);
        drain(s);                                    // chunk c - 2: its rows, inputs and staging are free after this
        uint8_t *h_reads = h_reads_[s].get(), *h_refs = h_refs_[s].get(), *d_reads = d_reads_[s].get(), *d_refs = d_refs_[s].get();
        auto t0 = std::chrono::steady_clock::now();
        gather(reads + begin, refs + begin, cnt, h_reads, h_refs, threads);
        host_stats_.gather_ms += ms_between(t0, std::chrono::steady_clock::now());
        hip_check(hipMemcpyAsync(d_reads, h_reads, (size_t)cnt * R_, hipMemcpyHostToDevice, copy_in), "H2D reads");
        hip_check(hipMemcpyAsync(d_refs, h_refs, (size_t)cnt * F_, hipMemcpyHostToDevice, copy_in), "H2D refs");
        hip_check(hipEventRecord(in_done_[s].get(), copy_in), "hipEventRecord");
        hip_check(hipStreamWaitEvent(kernels, in_done_[s].get(), 0), "hipStreamWaitEvent");
        // records only: the ops wait for the chunk's scan.  The walk (and the encoder behind it) of this chunk runs on the
        // helper stream beside the fill of the next one, as in align_host.
        const CigarSink sink{d_cig_recs_[s].get(), nullptr, 1, extended};
        bool chained = false;
        {
            ScopedSink<CigarSink> scoped(cigar_, &sink);
            if (!(small && route == AlignRoute::Fused && align_fused(alg, cnt, d_reads, d_refs, d_cig_rows_[s].get(), d_cig_idx_[s].get(), kernels))) {
                const WalkChain chain{s, chunk, nullptr, nullptr};
                chained = align_device(opt, cnt, d_reads, d_refs, d_cig_rows_[s].get(), d_cig_idx_[s].get(), kernels, &chain);
            }
        }
        hipStream_t tail = chained ? trace_stream_.get() : kernels;
        launch_cigar_scan(d_cig_recs_[s].get(), d_cig_offsets_[s].get(), cnt, tail);
        hip_check(hipMemcpyAsync(h_cig_total_.get() + s, d_cig_offsets_[s].get() + cnt, sizeof(long long), hipMemcpyDeviceToHost, tail), "D2H op total");
        hip_check(hipEventRecord(kernels_done_[s].get(), tail), "hipEventRecord");
        pend[s].begin = begin;
        pend[s].cnt = cnt;
        pend[s].active = true;
        if (chunk_no > 0) emit(s ^ 1);               // (the device has this chunk's fill to do meanwhile)
    }
    const int last = (int)((chunk_no - 1) & 1);
    emit(last);
    drain(last ^ 1);
    drain(last);
    quiesce.armed = false;
    *ops_needed = total_ops;
    return total_ops <= ops_cap;
}

}  // namespace valign
