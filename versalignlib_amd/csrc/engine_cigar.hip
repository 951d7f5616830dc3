// engine_cigar.hip -- Engine: the compact result format (include/valign_hip.h: valign_hip_aln records + 32-bit CIGAR ops).
// The alignment paths of engine_align.hip run unchanged into an engine-owned rows scratch; cigar_encode_kernel
// (cigar_kernels.hip.h) reads each part's rows behind its walk.  The rows never cross PCIe.
// Also here, once, for align_cigar_host and for the host calls of engine_span_cigar.hip and engine_extend_align.hip: the
// packed delivery of a chunk -- argument checks, raw staging, scan and op total, the emit pass, ONE copy back, unpacking (its
// pure half: PackedLayout, OpsBudget and HostPacker::unpack_packed of host_pipeline.h) -- and the one launch of cigar_encode_kernel,
// at the caller's row pitch.
#define VALIGN_TU_CIGAR 1
#include "engine.hip.h"

namespace valign {

void Engine::launch_cigar_args(hipStream_t stream, CigarArgs &a, int pitch) {
    a.AL = pitch;
    launch_encoder(stream, a, cigar_encode_kernel<16>, cigar_encode_kernel<64>, "hipLaunchKernel(cigar_encode_kernel)");
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
    launch_cigar_args(stream, a, R_ + F_);
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
        cig_pack_[s].recs.reserve(sizeof(CigarRec) * (size_t)pairs, "alignment records");
        cig_pack_[s].offsets.reserve(sizeof(long long) * ((size_t)pairs + 1), "op offsets");
        cigar_pairs_[s] = pairs;
    }
    h_cig_total_.reserve(sizeof(long long) * 2, "op totals");
}

// ---- packed delivery: the steps of a chunk that align_cigar_host, align_span_host and align_extend_host share ----

void Engine::check_packed_device_args(int extended, int ops_stride, const void *d_recs, const void *d_ops) {
    if (extended != 0 && extended != 1) throw std::runtime_error("extended must be 0 (M) or 1 (= / X)");
    if (ops_stride < 1) throw std::runtime_error("ops_stride must be >= 1");
    if (!d_recs || !d_ops) throw std::runtime_error("null result buffer");
}

void Engine::check_packed_host_args(int extended, int n, const void *recs, const void *ops, long long ops_cap, const long long *offsets,
                                    const long long *ops_needed) {
    if (extended != 0 && extended != 1) throw std::runtime_error("extended must be 0 (M) or 1 (= / X)");
    if (!recs || !offsets || !ops_needed || (!ops && ops_cap > 0)) throw std::runtime_error("null result buffer");
    if (n < 0 || ops_cap < 0) throw std::runtime_error("negative size");
}

void Engine::stage_raw_chunk(int slot, hipStream_t stream, const char *const *reads, const char *const *refs, long long cnt, int threads) {
    uint8_t *h_reads = h_reads_[slot].get(), *h_refs = h_refs_[slot].get();
    auto t0 = std::chrono::steady_clock::now();
    gather(reads, refs, cnt, h_reads, h_refs, threads);
    host_stats_.gather_ms += ms_between(t0, std::chrono::steady_clock::now());
    hip_check(hipMemcpyAsync(d_reads_[slot].get(), h_reads, (size_t)cnt * R_, hipMemcpyHostToDevice, stream), "H2D reads");
    hip_check(hipMemcpyAsync(d_refs_[slot].get(), h_refs, (size_t)cnt * F_, hipMemcpyHostToDevice, stream), "H2D refs");
}

void Engine::finish_count_pass(CigarPack &pack, long long cnt, long long *h_total_slot, hipStream_t stream) {
    launch_cigar_scan(pack.recs.get(), pack.offsets.get(), cnt, stream);
    hip_check(hipMemcpyAsync(h_total_slot, pack.offsets.get() + cnt, sizeof(long long), hipMemcpyDeviceToHost, stream), "D2H op total");
}

void Engine::emit_packed(CigarPack &pack, const PackedLayout &layout, const EmitLaunch &fill_and_launch, const void *d_extra, hipStream_t stream) {
    const size_t bytes = layout.bytes();
    if (bytes > pack.h_out.bytes()) {                     // (the last copy out of it was waited for before the pack was reused)
        pack.h_out.reserve(bytes + bytes / 4, "packed alignment results");
        pack.out.reserve(bytes + bytes / 4, "packed alignment results");
    }
    uint8_t *out = pack.out.get();
    const uint8_t *src = reinterpret_cast<const uint8_t *>(pack.recs.get());
    if (layout.with_ops) {                              // emit pass: the ops at their offsets, the records in front
        fill_and_launch(reinterpret_cast<unsigned *>(out + layout.ops_at()), reinterpret_cast<CigarRec *>(out));
        src = out;
    } else if (d_extra) {
        hip_check(hipMemcpyAsync(out, pack.recs.get(), layout.rec_bytes, hipMemcpyDeviceToDevice, stream), "D2D records");
        src = out;
    }
    if (d_extra) hip_check(hipMemcpyAsync(out + layout.rec_bytes, d_extra, layout.extra_bytes, hipMemcpyDeviceToDevice, stream), "D2D extra records");
    hip_check(hipMemcpyAsync(pack.h_out.get(), src, bytes, hipMemcpyDeviceToHost, stream), "D2H records + ops");
    cigar_d2h_bytes_ += (long long)(bytes + sizeof(long long));
}

void Engine::drain_packed(const CigarPack &pack, const PackedLayout &layout, long long begin, CigarRec *recs, void *extra, unsigned *ops, long long *offsets,
                          int threads) {
    auto t0 = std::chrono::steady_clock::now();
    packer_.unpack_packed(layout, pack.h_out.get(), begin, recs, extra, ops, offsets, threads);
    host_stats_.drain_ms += ms_between(t0, std::chrono::steady_clock::now());
}

void Engine::align_cigar_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int extended, CigarRec *d_recs,
                                unsigned *d_ops, int ops_stride, hipStream_t stream) {
    ran_cigar_lanes_ = 0;                   // (a refused call reports no encoder)
    check_packed_device_args(extended, ops_stride, d_recs, d_ops);
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
        ScopedSink scoped(cigar_, &sink);
        align_device(opt, cnt, d_reads + (size_t)begin * R_, d_refs + (size_t)begin * F_, d_cig_rows_[0].get(), d_cig_idx_[0].get(), stream);
    }
}

// Host pointers in, packed results out, on the two-slot pipeline of align_host: the fill of chunk c + 1 (kernels stream) beside
// the emit pass and the copy back of chunk c (copy_out stream) and the drain of chunk c - 1.  The steps inside a chunk are the
// shared ones above; this schedule is this call's own.
bool Engine::align_cigar_host(int opt, int n, const char *const *reads, const char *const *refs, int extended, CigarRec *recs,
                              unsigned *ops, long long ops_cap, long long *offsets, long long *ops_needed, int threads) {
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
    ran_align_fill_ = "none";
    ran_align_geo_ = nullptr;
    ran_result_format_ = "cigar";           // (before the refusals: a refused call must not report the format of an earlier one)
    const int AL = R_ + F_;
    const RouteFacts facts = route_facts(true);
    const AlignRoute route = valign::align_route(rule_inputs(), alg, facts);       // (refusals leave here)
    const bool by_strips = strip_chunks(route, facts);
    // (the chunks of align_host: same launches, same rounds)
    const size_t chunk_bytes = by_strips && !dbg_.on("align_chunk_bytes") ? std::max<size_t>(align_chunk_bytes_, 384u << 20) : align_chunk_bytes_;
    const long long chunk = std::min<long long>(packed_chunk_pairs(chunk_bytes), n);
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
        long long begin = 0, cnt = 0;
        bool active = false;
        PackedLayout layout;
    } pend[2];
    OpsBudget budget{ops_cap};
    // Chunk in slot s: its records and scanned offsets are on the device and its op total is on its way.  Size the packed
    // output, emit the ops beside the records (copy_out stream: beside the next chunk's fill) and start ONE copy back.
    auto emit = [&](int s) {
        Pending &p = pend[s];
        auto t0 = std::chrono::steady_clock::now();
        hip_check(hipEventSynchronize(kernels_done_[s].get()), "hipEventSynchronize");
        host_stats_.wait_ms += ms_between(t0, std::chrono::steady_clock::now());
        const long long total = h_cig_total_.get()[s];
        p.layout = PackedLayout(p.cnt, 0, total, budget.add(total));
        emit_packed(cig_pack_[s], p.layout, [&](unsigned *d_ops, CigarRec *recs_out) {
            CigarArgs a = emit_args<CigarArgs>(cig_pack_[s], d_cig_rows_[s].get(), d_cig_idx_[s].get(), p.cnt, extended, d_ops, recs_out);
            launch_cigar_args(copy_out, a, AL);
        }, nullptr, copy_out);
        hip_check(hipEventRecord(slot_done_[s].get(), copy_out), "hipEventRecord");
    };
    auto drain = [&](int s) {
        Pending &p = pend[s];
        if (!p.active) return;
        auto t0 = std::chrono::steady_clock::now();
        hip_check(hipEventSynchronize(slot_done_[s].get()), "hipEventSynchronize");
        host_stats_.wait_ms += ms_between(t0, std::chrono::steady_clock::now());
        drain_packed(cig_pack_[s], p.layout, p.begin, recs, nullptr, ops, offsets, threads);
        p.active = false;
    };
    long long chunk_no = 0;
    for (long long begin = 0; begin < n; begin += chunk, ++chunk_no) {
        const int s = (int)(chunk_no & 1);
        const long long cnt = std::min<long long>(chunk, n - begin);
        drain(s);                                    // chunk c - 2: its rows, inputs and staging are free after this
        stage_raw_chunk(s, copy_in, reads + begin, refs + begin, cnt, threads);
        hip_check(hipEventRecord(in_done_[s].get(), copy_in), "hipEventRecord");
        hip_check(hipStreamWaitEvent(kernels, in_done_[s].get(), 0), "hipStreamWaitEvent");
        const uint8_t *d_reads = d_reads_[s].get(), *d_refs = d_refs_[s].get();
        // records only: the ops wait for the chunk's scan.  The walk (and the encoder behind it) of this chunk runs on the
        // helper stream beside the fill of the next one, as in align_host.
        const CigarSink sink{cig_pack_[s].recs.get(), nullptr, 1, extended};
        bool chained = false;
        {
            ScopedSink scoped(cigar_, &sink);
            if (!(small && route == AlignRoute::Fused && align_fused(alg, cnt, d_reads, d_refs, d_cig_rows_[s].get(), d_cig_idx_[s].get(), kernels))) {
                const WalkChain chain{s, chunk, nullptr, nullptr};
                chained = align_device(opt, cnt, d_reads, d_refs, d_cig_rows_[s].get(), d_cig_idx_[s].get(), kernels, &chain);
            }
        }
        hipStream_t tail = chained ? trace_stream_.get() : kernels;
        finish_count_pass(cig_pack_[s], cnt, h_cig_total_.get() + s, tail);
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
    *ops_needed = budget.total;
    return budget.fits();
}

}  // namespace valign

