// engine_extend_align.hip -- Engine: extension alignments (include/valign_hip.h: valign_hip_align_extend_*): per pair the alignment
// from the anchor before read[0] and ref[0] to the end cell the end-bonus rule picks, as a valign_hip_aln record and CIGAR ops, and
// the pair's extension record where asked for.  extend_align_choice (cell_rules.h) decides what is refused; a chunk runs
// align_extend_fill_kernel (extend_align_kernels.hip.h) into the pointer scratch alignments use, extend_walk_kernel into the CIGAR
// rows scratch at a row pitch of R + F + 1, and cigar_encode_kernel behind it (launch_cigar_args of engine_cigar.hip, at that pitch).
// extend_walk_kernel (not a template) is defined in this translation unit.
// Where the rule answers Band (extend_band_align = 1 under a band with extend_band = 1) a chunk is extend_band_align_chunk: the
// lengths pre-pass and the boundary rows of banded extension scores (extend_band_sweep, engine_extend.hip), one launch of
// align_extend_band_fill_kernel per strip into the same pointer scratch, extend_band_ends_kernel, extend_band_walk_kernel and the
// encoder (extend_band_align_kernels.hip.h; its two fill instances and the two other kernels are defined here).  Chunk sizes, the
// scratch and both entry points are shared: only the chunk body differs.  The host entry delivers through the packed path of
// engine_cigar.hip, the extension records between the records and the ops.
// Under extend_zdrop > 0 the rule is extend_zdrop_align_choice (extend_zdrop.h), which wraps extend_align_choice(...): the Band route
// or nothing, its fill the ZDROP instance, the ends kernel with the chunk's drop rows.  Under extend_zdrop_rows = 1 the rule is
// extend_zdrop_rows_align_choice, which wraps extend_zdrop_align_choice(in, alg, facts, G, K, Z): an unbanded call on the register
// route runs the fill's ZDROP instance (Geometry::extend_align_zdrop) -- same plan, scratch, walk and encoder.
#define VALIGN_TU_EXTEND_ALIGN 1
#include "engine.hip.h"
#include "extend_band_align_kernels.hip.h"

namespace valign {

const LaunchPlan &Engine::extend_align_plan_for(int alg, ExtendAlignChoice &choice) {
    const LaunchPlan &base = align_base_plan();
    const PlacedFacts facts = placed_facts();
    RuleInputs in = rule_inputs();
    in.no_f16 = true;                   // int16 cells
    choice = extend_zdrop_rows_align_choice(in, alg, facts, base.geo ? base.geo->G : 0, base.geo ? base.geo->K : 0, extend_zdrop_, extend_zdrop_rows_);
    if (choice.route == PlacedRoute::Refused) throw std::runtime_error(choice.reason);
    if (choice.route == kPlacedRouteBand) return base;                  // (nothing launches on the plan)
    if (base.geo->extend_align(sc_.affine ? 1 : 0) && base.geo->extend_align_zdrop(sc_.affine ? 1 : 0)) return base;
    if (!fallback_plan_.geo) fallback_plan_ = choose_plan(R_, F_, 0, 0, false, true);
    if (fallback_plan_.long_mode || !fallback_plan_.geo->extend_align(sc_.affine ? 1 : 0)) throw std::runtime_error("no extension-alignment kernel for this mode");
    choice = extend_zdrop_rows_align_choice(in, alg, facts, fallback_plan_.geo->G, fallback_plan_.geo->K, extend_zdrop_, extend_zdrop_rows_);
    return fallback_plan_;
}

long long Engine::extend_align_chunk_pairs(const LaunchPlan &plan, const ExtendAlignChoice &choice, long long n, size_t rows_cap) const {
    const long long ppw = plan.pairs_per_wave, ppb = ppw * plan.waves_per_block;
    size_t free_b = 0, total_b = 0;
    hip_check(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
    // the pointer scratch's bound is the one alignments size theirs by (align_parts.h), under pointer_scratch_cap_mb
    size_t ptr_cap = std::min<size_t>(64ull << 30, std::max<size_t>((free_b + d_ptr_.bytes()) / 2, 256ull << 20));
    if (scratch_cap_mb_ > 0) ptr_cap = std::min<size_t>(ptr_cap, (size_t)scratch_cap_mb_ << 20);
    const long long by_ptr = (long long)(ptr_cap / (size_t)choice.wave_ptr_bytes) * ppw;
    const long long by_rows = (long long)(rows_cap / (2 * ((size_t)R_ + F_ + 1)));
    long long chunk = std::min(by_ptr, by_rows);
    if (choice.route == kPlacedRouteBand) {
        // a wave is a pair-of-pairs; the boundary rows of the chunk's strips lie in the strip scratch, under its cap
        const StripPlan strips = extend_band_sweep().plan;
        const size_t rows_per_pp = (size_t)2 * strips.row_sets * strips.row_dwords * 4;
        const long long by_ptr_pp = (long long)(ptr_cap / (size_t)choice.wave_ptr_bytes) * 2;
        chunk = std::min({by_ptr_pp, by_rows, strip_chunk_pairs(strip_scratch_cap(free_b + d_placed_rows_.bytes(), scratch_cap_mb_), rows_per_pp, n)});
        chunk = std::max<long long>(2, chunk / 2 * 2);              // whole waves, at least one
        return std::min(chunk, n);
    }
    chunk = std::max(ppb, chunk / ppb * ppb);           // whole blocks, at least one
    return std::min(chunk, n);
}

void Engine::ensure_extend_align_rows(int slots, long long pairs, hipStream_t stream) {
    // ensure_cigar_scratch sizes rows of R + F bytes: as many such pairs as hold `pairs` pairs at the walk's pitch
    const size_t AL = (size_t)R_ + F_;
    const long long as_pairs = AL ? (long long)(((size_t)pairs * 2 * (AL + 1) + 2 * AL - 1) / (2 * AL)) : pairs;
    ensure_cigar_scratch(slots, std::max(as_pairs, pairs), stream);
}

void Engine::ensure_extend_align_scratch(const LaunchPlan &plan, const ExtendAlignChoice &choice, long long pairs, hipStream_t stream) {
    ensure_extend_align_rows(1, pairs, stream);
    if (choice.route != kPlacedRouteBand) {
        ensure_trace_scratch(pairs, (size_t)(choice.wave_ptr_bytes / (plan.pairs_per_wave / 2)), plan.pairs_per_wave, stream);
        return;
    }
    ensure_trace_scratch(pairs, (size_t)choice.wave_ptr_bytes, 2, stream);
    const PlacedSweep sweep = extend_band_sweep();
    const size_t rows = (size_t)((pairs + 1) / 2) * 2 * sweep.plan.row_sets * sweep.plan.row_dwords * 4, per_pair = sweep.pair_bytes * (size_t)(pairs + 1);
    if (rows > d_placed_rows_.bytes() || per_pair > d_placed_ends_.bytes()) {
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");          // nothing may still read the old scratch
        d_placed_rows_.reserve(rows, sweep.rows_label);
        d_placed_ends_.reserve(per_pair, "extension partial records and trimmed lengths");
    }
}

// The Band route.  The strip loop is score_placed_strips' (engine_placed.hip) with the fill in the kernel's place and the pointer
// regions in StripArgs.ends; what follows the last strip is this route's own.
void Engine::extend_band_align_chunk(const ExtendAlignChoice &choice, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int end_bonus, int extended,
                                     CigarRec *recs, unsigned *ops, int ops_stride, ExtendRec *d_extend, int slot, hipStream_t stream) {
    constexpr int K = kExtendWideK;
    const PlacedSweep sweep = extend_band_sweep();
    const StripPlan &plan = sweep.plan;
    const long long waves = (n + 1) / 2;
    if (waves > 0x7FFFFFFFll) throw std::runtime_error("batch too large for one launch");
    const size_t bytes_per_pp = (size_t)2 * plan.row_sets * plan.row_dwords * 4;
    if ((size_t)waves * (size_t)choice.wave_ptr_bytes > d_ptr_.bytes() || sizeof(EndCell) * (size_t)n > d_ends_.bytes() ||
        (size_t)n * 2 * ((size_t)R_ + F_ + 1) > d_cig_rows_[slot].bytes() || (size_t)waves * bytes_per_pp > d_placed_rows_.bytes() ||
        sweep.pair_bytes * (size_t)n > d_placed_ends_.bytes())
        throw std::runtime_error("extension alignments: chunk larger than its scratch");
    const bool zdrop = extend_zdrop_on(extend_zdrop_);
    const void *plain = sc_.affine ? (const void *)align_extend_band_fill_kernel<K, true> : (const void *)align_extend_band_fill_kernel<K, false>;
    const void *dropping = sc_.affine ? (const void *)align_extend_band_fill_zdrop_kernel<K, true> : (const void *)align_extend_band_fill_zdrop_kernel<K, false>;
    const void *fn = zdrop ? dropping : plain;
    raise_block_lds(fn, sweep.lds.total);
    const size_t f_rows = plan.f_rows_at(waves), slot_dwords = plan.row_sets * f_rows;
    StripArgs first{};
    for (int s = 0; s < plan.strips; ++s) {
        StripArgs a = strip_args(d_reads, d_refs, n, plan, sweep.lds, s, d_placed_rows_.get(), (size_t)((s + 1) & 1) * slot_dwords, (size_t)(s & 1) * slot_dwords,
                                 f_rows, d_placed_ends_.get(), nullptr);
        sweep.bind(a, n);                                           // ptr: the partial records, first_bad: the trimmed lengths behind them
        if (s == 0) {
            sweep.open(a, 0, stream);                               // the lengths pre-pass
            first = a;
        }
        a.ends = reinterpret_cast<EndCell *>(d_ptr_.get());         // the chunk's pointer regions
        void *kargs[] = {&a};
        hip_check(hipLaunchKernel(fn, dim3((unsigned)waves), dim3(kWave), kargs, (size_t)sweep.lds.total, stream), "hipLaunchKernel(align_extend_band_fill_kernel)");
    }
    hipLaunchKernelGGL(extend_band_ends_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const int *)first.ptr, first.first_bad, d_extend, d_ends_.get(), n,
                       choice.band_half, end_bonus, zdrop ? extend_drop_rows(first) : nullptr);
    hip_check(hipGetLastError(), "hipLaunchKernel(extend_band_ends_kernel)");
    ExtendWalkArgs t{};
    t.reads = d_reads;
    t.refs = d_refs;
    t.ptr = d_ptr_.get();
    t.ends = d_ends_.get();
    t.rows = d_cig_rows_[slot].get();
    t.idx = d_cig_idx_[slot].get();
    t.n = n;
    t.R = R_;
    t.F = F_;
    t.blocks8 = choice.blocks8;
    t.affine = sc_.affine ? 1 : 0;
    t.pitch = R_ + F_ + 1;
    t.band_half = choice.band_half;
    hipLaunchKernelGGL(extend_band_walk_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, t);
    hip_check(hipGetLastError(), "hipLaunchKernel(extend_band_walk_kernel)");
    CigarArgs a{};
    a.rows = t.rows;
    a.idx = t.idx;
    a.ends = d_ends_.get();
    a.recs = recs;
    a.ops = ops;
    a.ops_stride = ops_stride;
    a.n = n;
    a.extended = extended;
    launch_cigar_args(stream, a, t.pitch);
    ran_extend_align_ = ran_placed_name(kPlacedRouteBand);
    align_ptr_bytes_per_pair_ = choice.wave_ptr_bytes / 2;
}

void Engine::extend_align_chunk(const LaunchPlan &plan, const ExtendAlignChoice &choice, long long n, const uint8_t *d_reads, const uint8_t *d_refs,
                                int end_bonus, int extended, CigarRec *recs, unsigned *ops, int ops_stride, ExtendRec *d_extend, int slot,
                                hipStream_t stream) {
    ++ran_extend_align_chunks_;
    if (choice.route == kPlacedRouteBand)
        return extend_band_align_chunk(choice, n, d_reads, d_refs, end_bonus, extended, recs, ops, ops_stride, d_extend, slot, stream);
    const int G = plan.geo->G, K = plan.geo->K;
    const long long ppw = plan.pairs_per_wave, ppb = ppw * plan.waves_per_block;
    const long long blocks = (n + ppb - 1) / ppb;
    if (blocks > 0x7FFFFFFFll) throw std::runtime_error("batch too large for one launch");
    if ((size_t)((n + ppw - 1) / ppw) * (size_t)choice.wave_ptr_bytes > d_ptr_.bytes() || sizeof(EndCell) * (size_t)n > d_ends_.bytes() ||
        (size_t)n * 2 * ((size_t)R_ + F_ + 1) > d_cig_rows_[slot].bytes())
        throw std::runtime_error("extension alignments: chunk larger than its scratch");
    ExtendAlignArgs f{};
    f.reads = d_reads;
    f.refs = d_refs;
    f.ptr = d_ptr_.get();
    f.ends = d_ends_.get();
    f.extend = d_extend;
    f.n = n;
    f.R = R_;
    f.F = F_;
    f.blocks8 = choice.blocks8;
    f.end_bonus = end_bonus;
    put_lds(f, plan.lds);
    put_scoring(f);
    // keys extend_zdrop > 0 and extend_zdrop_rows = 1 (the route is Rows: without the second key the rule refused the call)
    const bool dropping = extend_zdrop_rows_ && extend_zdrop_on(extend_zdrop_);
    f.Z = dropping ? extend_zdrop_ : 0;
    ran_extend_zdrop_ = f.Z;
    ran_extend_zdrop_rows_ = dropping;
    const void *fn = dropping ? plan.geo->extend_align_zdrop(sc_.affine ? 1 : 0) : plan.geo->extend_align(sc_.affine ? 1 : 0);
    ran_extend_align_geo_ = plan.geo;
    const int block_lds = plan.lds.total * plan.waves_per_block;
    raise_block_lds(fn, block_lds);
    void *fargs[] = {&f};
    hip_check(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(plan.waves_per_block * kWave), fargs, (size_t)block_lds, stream),
              "hipLaunchKernel(align_extend_fill_kernel)");
    ExtendWalkArgs t{};
    t.reads = d_reads;
    t.refs = d_refs;
    t.ptr = d_ptr_.get();
    t.ends = d_ends_.get();
    t.rows = d_cig_rows_[slot].get();
    t.idx = d_cig_idx_[slot].get();
    t.n = n;
    t.R = R_;
    t.F = F_;
    t.G = G;
    t.K = K;
    t.blocks8 = choice.blocks8;
    t.affine = sc_.affine ? 1 : 0;
    t.pitch = R_ + F_ + 1;
    hipLaunchKernelGGL(extend_walk_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, t);
    hip_check(hipGetLastError(), "hipLaunchKernel(extend_walk_kernel)");
    CigarArgs a{};
    a.rows = t.rows;
    a.idx = t.idx;
    a.ends = d_ends_.get();
    a.recs = recs;
    a.ops = ops;
    a.ops_stride = ops_stride;
    a.n = n;
    a.extended = extended;
    launch_cigar_args(stream, a, t.pitch);
    ran_extend_align_ = ran_placed_name(PlacedRoute::Rows);
    align_ptr_bytes_per_pair_ = choice.wave_ptr_bytes / ppw;           // (the call's own, as on the Band route: not the last other alignment's)
}

void Engine::align_extend_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int end_bonus, int extended, CigarRec *d_recs,
                                 unsigned *d_ops, int ops_stride, ExtendRec *d_extend, hipStream_t stream) {
    ran_extend_align_ = "none";
    ran_extend_align_geo_ = nullptr;
    ran_extend_align_chunks_ = 0;
    ran_cigar_lanes_ = 0;
    ran_extend_zdrop_ = 0;
    ran_extend_zdrop_rows_ = false;
    check_packed_device_args(extended, ops_stride, d_recs, d_ops);
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;          // reference: unsupported mode is a silent no-op
    ExtendAlignChoice choice;
    const LaunchPlan &plan = extend_align_plan_for(alg, choice);        // (refusals leave here, before anything is launched)
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (choice.route == kPlacedRouteBand) start_extend_zdrop(stream);
    ran_result_format_ = "cigar";
    const size_t rows_cap = (size_t)std::max<long long>(1, dbg_.value("cigar_rows_mb", 512)) << 20;
    const long long chunk = extend_align_chunk_pairs(plan, choice, n, rows_cap);
    ensure_extend_align_scratch(plan, choice, chunk, stream);
    for (long long begin = 0; begin < n; begin += chunk)          // (stream order: the next chunk reuses the scratch behind this one's encoder)
        extend_align_chunk(plan, choice, std::min(chunk, n - begin), d_reads + (size_t)begin * R_, d_refs + (size_t)begin * F_, end_bonus, extended,
                           d_recs + begin, d_ops + (size_t)begin * ops_stride, ops_stride, d_extend ? d_extend + begin : nullptr, 0, stream);
}

// Host pointers in, packed results out.  Chunk after chunk on streams_[0], each waited for: the raw staging, the chunk above with
// a records-only sink (count pass), then the packed delivery of engine_cigar.hip -- scan, op total, emit pass at the scanned
// offsets beside the records (and, where asked for, the extension records between them), ONE copy back, unpacking -- with the
// encoder at the walk's row pitch as the emit pass.
bool Engine::align_extend_host(int opt, int n, const char *const *reads, const char *const *refs, int end_bonus, int extended, CigarRec *recs,
                               unsigned *ops, long long ops_cap, long long *offsets, long long *ops_needed, ExtendRec *extend, int threads) {
    ran_extend_align_ = "none";
    ran_extend_align_geo_ = nullptr;
    ran_extend_align_chunks_ = 0;
    ran_cigar_lanes_ = 0;
    ran_extend_zdrop_ = 0;
    ran_extend_zdrop_rows_ = false;
    check_packed_host_args(extended, n, recs, ops, ops_cap, offsets, ops_needed);
    const int alg = opt & 0xF;
    if (alg > 1) return true;                       // (the same silent no-op as every entry point)
    offsets[0] = 0;
    *ops_needed = 0;
    cigar_d2h_bytes_ = 0;
    if (n == 0) return true;
    if (!reads || !refs) throw std::runtime_error("null sequence array");
    ExtendAlignChoice choice;
    const LaunchPlan &plan = extend_align_plan_for(alg, choice);        // (refusals leave here, before anything is staged)
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ran_result_format_ = "cigar";
    // (the chunks of align_cigar_host, inside the bounds of the pointer and rows scratch)
    long long chunk = std::min<long long>(packed_chunk_pairs(align_chunk_bytes_),
                                          extend_align_chunk_pairs(plan, choice, n, (size_t)std::max<long long>(1, dbg_.value("cigar_rows_mb", 512)) << 20));
    if (choice.route == kPlacedRouteBand && chunk < n) chunk = std::max<long long>(2, chunk / 2 * 2);       // whole waves
    reset_pipeline();
    ensure_staging(chunk);
    threads = std::min(std::max(threads, 1), 64);
    hipStream_t st = streams_[0].get();
    if (choice.route == kPlacedRouteBand) start_extend_zdrop(st);
    ensure_extend_align_scratch(plan, choice, chunk, st);
    if (extend) d_extend_align_recs_.reserve(sizeof(ExtendRec) * (size_t)chunk, "extension records");
    ExtendRec *d_extend = extend ? d_extend_align_recs_.get() : nullptr;
    CigarPack &pack = cig_pack_[0];
    host_stats_ = HostStats{};
    struct Quiesce {            // an error part-way leaves nothing in flight
        hipStream_t st;
        bool armed = true;
        ~Quiesce() {
            if (armed) (void)hipStreamSynchronize(st);
        }
    } quiesce{st};
    auto wait = [&] {
        auto t0 = std::chrono::steady_clock::now();
        hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
        host_stats_.wait_ms += ms_between(t0, std::chrono::steady_clock::now());
    };
    OpsBudget budget{ops_cap};
    for (long long begin = 0; begin < n; begin += chunk) {
        const long long cnt = std::min<long long>(chunk, n - begin);
        stage_raw_chunk(0, st, reads + begin, refs + begin, cnt, threads);
        // records only: the ops wait for the chunk's scan
        extend_align_chunk(plan, choice, cnt, d_reads_[0].get(), d_refs_[0].get(), end_bonus, extended, pack.recs.get(), nullptr, 1, d_extend, 0, st);
        finish_count_pass(pack, cnt, h_cig_total_.get(), st);
        wait();
        const long long total = h_cig_total_.get()[0];
        const PackedLayout layout(cnt, extend ? sizeof(ExtendRec) : 0, total, budget.add(total));
        emit_packed(pack, layout, [&](unsigned *d_ops, CigarRec *recs_out) {
            CigarArgs a = emit_args<CigarArgs>(pack, d_cig_rows_[0].get(), d_cig_idx_[0].get(), cnt, extended, d_ops, recs_out);
            launch_cigar_args(st, a, R_ + F_ + 1);      // the walk's row pitch
        }, d_extend, st);
        wait();
        drain_packed(pack, layout, begin, recs, extend ? extend + begin : nullptr, ops, offsets, threads);
    }
    quiesce.armed = false;
    *ops_needed = budget.total;
    return budget.fits();
}

}  // namespace valign
