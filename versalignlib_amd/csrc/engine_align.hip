// engine_align.hip -- Engine: compute_alignments (reference: src/Kernels/default/DefaultKernel.cpp:21-50, 204-525) -- fill +
// traceback launches, row strips for long reads, the fused small-batch launch, and the host-pointer pipeline.  traceback_kernel
// and first_invalid_kernel (not templates) are defined in this translation unit.
#define VALIGN_TU_ALIGN 1
#include "engine.hip.h"
#include "versalign_plugin_abi.h"

namespace valign {

// compute_alignments for reads beyond one register sweep (strip_kernels.hip.h): a wave per pair-of-pairs, K rows per lane.
// The one place a strip kernel is instantiated: the instance of (mode, pass) number I -- bit 0 the algorithm, then int32
// cells, affine gaps, SSE tie-breaks, the band; above them the checkpointed pass (kCkptNone / kCkptForward / kCkptRefill) --
// where strip_instance_exists (strip_plan.h) says it is compiled, null elsewhere.
constexpr int kStripModeBits = 5, kStripInstances = 3 << kStripModeBits;
template <int K, int I>
const void *strip_instance() {
    constexpr int ALG = I & 1, CKPT = I >> kStripModeBits;
    constexpr bool WIDE = (I & 2) != 0, AFFINE = (I & 4) != 0, SSE = (I & 8) != 0, BAND = (I & 16) != 0;
    if constexpr (!strip_instance_exists(K, StripMode{ALG, AFFINE, SSE, WIDE, BAND, CKPT != kCkptNone})) return nullptr;
    else if constexpr (WIDE) return (const void *)&align_strip_wide_kernel<K, ALG, AFFINE, SSE, BAND>;
    else return (const void *)&align_strip_kernel<K, ALG, AFFINE, SSE, BAND, CKPT>;
}
// ckpt_pass (checkpointed modes): 0 the forward pass, 1 the re-fill
template <int K, int... I>
const void *strip_kernel_in(const StripMode &m, int ckpt_pass, std::integer_sequence<int, I...>) {
    static const void *const instances[] = {strip_instance<K, I>()...};
    const int pass = m.ckpt ? (ckpt_pass ? kCkptRefill : kCkptForward) : kCkptNone;
    return instances[m.alg | m.wide << 1 | m.affine << 2 | m.sse << 3 | m.band << 4 | pass << kStripModeBits];
}
template <int K>
const void *strip_kernel(const StripMode &m, int ckpt_pass) {
    return strip_kernel_in<K>(m, ckpt_pass, std::make_integer_sequence<int, kStripInstances>());
}
struct StripGeometry {
    int K;
    WaveLds lds;            // the profile of 64 K rows and the ring of slab numbers: no term in the shape
    const void *(*kernel)(const StripMode &, int ckpt_pass);
};
template <int K>
constexpr StripGeometry strip_geometry{K, {StripLds<K>::kRing, 0, StripLds<K>::kTotal}, &strip_kernel<K>};
constexpr StripGeometry kStripGeometries[] = {strip_geometry<kStripKs[0]>, strip_geometry<kStripKs[1]>, strip_geometry<kStripKs[2]>};
static_assert(sizeof(kStripKs) == 3 * sizeof(int), "a row per K that strip_plan.h chooses among");

// Small batches: fill + traceback in one launch, pointer stream in LDS (align_fill_tag_kernel<..., FUSED>)
struct FusedGeometry {
    int G, K;
    WaveLds (*lds)(int R, int F);
    int (*total)(int wave_lds, int R, int F, int blocks8);
    const void *kernel[2];
};
template <int G, int K>
constexpr FusedGeometry make_fused() {
    return FusedGeometry{G, K, &wave_lds<G, K>,
                         [](int wl, int R, int F, int b8) { return fused_lds<G, K>(wl, R, F, b8).total; },
                         {(const void *)&align_fill_tag_kernel<G, K, kAlgSW, false, false, true>,
                          (const void *)&align_fill_tag_kernel<G, K, kAlgNW, false, false, true>}};
}
// (32 x 2 / 32 x 4: few rows per lane -- the shortest dependent chain per step, which is what a single-wave call costs)
// (64 x 4: a whole wave per pair-of-pairs -- the one geometry whose pointer stream fits LDS at 150 x 500, 83 KB: a
// 1,000-pair compute_alignments call of that shape is ONE launch instead of memset + fill + a traceback that chases
// pointers through HBM, 600 -> ~200 us)
static const FusedGeometry kFusedGeometries[] = {make_fused<8, 4>(), make_fused<16, 4>(), make_fused<32, 2>(), make_fused<16, 8>(),
                                                 make_fused<32, 4>(), make_fused<16, 10>(), make_fused<32, 8>(), make_fused<64, 4>()};

// The plan an alignment call of this mode runs on: the engine's own where its geometry carries the kernel the call needs;
// otherwise (a fallback kernel on a geometry compiled with the fast set only, kernel_instances.hip.h) the cheapest FULL
// geometry that fits the read -- same results, the sweep a few per cent longer.
const LaunchPlan &Engine::align_plan_for(int alg, FillChoice &choice) {
    const LaunchPlan &base = align_base_plan();
    choice = fill_choice(rule_inputs(), alg, base.geo->G, base.geo->K);
    if (base.geo->fill[alg][choice.kernel]) return base;
    if (!fallback_plan_.geo) fallback_plan_ = choose_plan(R_, F_, 0, 0, false, true);
    choice = fill_choice(rule_inputs(), alg, fallback_plan_.geo->G, fallback_plan_.geo->K);
    if (!fallback_plan_.geo->fill[alg][choice.kernel]) throw std::runtime_error("no alignment kernel for this mode");
    return fallback_plan_;
}

RouteFacts Engine::route_facts(bool small_call) const {
    int fused_rows = 0;
    for (const FusedGeometry &g : kFusedGeometries) fused_rows = std::max(fused_rows, g.G * g.K);
    // row strips: reads beyond one register sweep, and -- measured, profiles/r04_rate_sweep.txt -- reads of more than 1 024
    // rows, whose resident geometries (64 x 24 / 64 x 32: 34 to 53 KB of LDS) fill at 0.8-2.1 TCUPS where 12- or 16-row
    // strips at eight waves per CU do 1.6-2.3 (1 200 x 3 000: 41 / 74 ms -> 26 / 37 ms, linear / affine)
    const bool read_strips = align_base_plan().long_mode || (!force_g_ && !force_k_ && R_ > 1024);
    return RouteFacts{align_banded(), wide_align_, read_strips, no_fused_ || force_g_ || force_k_, small_call, fused_rows, trace_checkpoints_,
                      band_nw_, band_width_};
}

bool Engine::align_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs, uint8_t *d_rows,
                  short *d_idx, hipStream_t stream, const WalkChain *chain) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return false;
    ran_align_fill_ = "none";
    ran_align_geo_ = nullptr;
    ran_result_format_ = cigar_ ? "cigar" : "rows";
    align_ckpt_bytes_per_pair_ = 0;
    const AlignRoute route = valign::align_route(rule_inputs(), alg, route_facts(false));       // (throws what the mode refuses)
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (route != AlignRoute::Register) {
        ran_align_fill_ = ran_fill_name(route);
        align_strips_device(strip_mode(route, rule_inputs(), alg), n, d_reads, d_refs, d_rows, d_idx, stream);
        return false;
    }
    // the fill kernel of this mode -- and the geometry that has it: the plan's own, or the next full one (fallback kernels)
    FillChoice fc;
    const LaunchPlan &plan = align_plan_for(alg, fc);
    const bool affine_tagged = fc.affine_tagged, tagged = fc.tagged;
    const int G = plan.geo->G, K = plan.geo->K, AL = R_ + F_;
    const long long ppb = (long long)plan.pairs_per_wave * plan.waves_per_block;
    size_t free_b = 0, total_b = 0;
    hip_check(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
    const TraceScratch ts = size_trace_scratch(G, K, F_, sc_.affine, affine_tagged, ppb, free_b + d_ptr_.bytes(), scratch_cap_mb_, n,
                                               chain ? chain->chunk_pairs : 0, no_overlap_);
    const int blocks8 = ts.blocks8;
    const size_t bytes_per_pp = ts.bytes_per_pp;
    if (!ts.chained) chain = nullptr;                    // two regions do not fit: stream order
    if (!chain) chain_regions_busy_[0] = chain_regions_busy_[1] = false;
    ensure_trace_scratch(ts.chunk, bytes_per_pp, plan.pairs_per_wave, stream);
    align_ptr_bytes_per_pair_ = (long long)(bytes_per_pp / 2);
    const void *fn = plan.geo->fill[alg][fc.kernel];
    ran_align_fill_ = ran_fill_name(route, fc.kernel);
    ran_align_geo_ = plan.geo;
    const int block_lds = plan.lds.total * plan.waves_per_block;
    if (block_lds > kDefaultBlockLds)
        hip_check(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, block_lds),
                  "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    const bool overlap = !no_overlap_ && (double)n * R_ * F_ >= 1e10 && !chain;
    const std::vector<Part> parts = cut_parts(n, ts, chain ? chain->region : -1, overlap);      // (align_parts.h)
    const bool helper = (parts.size() > 1 && overlap) || chain;
    if (chain) {
        // rows are zeroed on the helper stream right before the walk that writes them (the caller has made sure the
        // previous user of d_rows is done: its copy-out event was waited for on the host)
        ensure_trace_stream();
    } else if (helper) {
        // the result rows are zeroed on the helper stream too (1.4 GB per million pairs of 150 x 500: the fills do not
        // touch them), behind whatever the caller's stream was still doing with them
        ensure_trace_stream();
        hip_check(hipEventRecord(entry_ev_.get(), stream), "hipEventRecord");
        hip_check(hipStreamWaitEvent(trace_stream_.get(), entry_ev_.get(), 0), "hipStreamWaitEvent");
        hip_check(hipMemsetAsync(d_rows, 0, (size_t)n * 2 * AL, trace_stream_.get()), "hipMemsetAsync(rows)");
    } else if (!chain) {
        hip_check(hipMemsetAsync(d_rows, 0, (size_t)n * 2 * AL, stream), "hipMemsetAsync(rows)");
    }
    bool region_used[2] = {chain && chain_regions_busy_[0], chain && chain_regions_busy_[1]};
    for (const Part &part : parts) {
        const long long begin = part.begin, cnt = part.cnt;
        unsigned *part_ptr = reinterpret_cast<unsigned *>(reinterpret_cast<unsigned char *>(d_ptr_.get()) + (size_t)(part.slot / 2) * bytes_per_pp);
        EndCell *part_ends = d_ends_.get() + part.slot;
        if (helper && region_used[part.region])          // the region's previous walk must be over before it is overwritten
            hip_check(hipStreamWaitEvent(stream, trace_done_[part.region].get(), 0), "hipStreamWaitEvent");
        FillArgs f{};
        put_sweep(f, d_reads + (size_t)begin * R_, d_refs + (size_t)begin * F_, cnt, blocks8, plan.lds);
        f.ptr = part_ptr;
        f.ends = part_ends;
        void *fargs[] = {&f};
        const long long blocks = (cnt + ppb - 1) / ppb;
        hip_check(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(plan.waves_per_block * kWave), fargs,
                                  (size_t)block_lds, stream),
                  "hipLaunchKernel(align_fill_kernel)");
        TraceArgs t = trace_args(alg, f.reads, f.refs, cnt, part_ptr, part_ends, d_rows + (size_t)begin * 2 * AL, d_idx + (size_t)begin * 4, G, K, G * K - R_, blocks8);
        t.tagged = affine_tagged ? 2 : ((tagged && !sse_policy_) ? 1 : 0);     // SSE tags are the stored states
        void *targs[] = {&t};
        hipStream_t walk_stream = stream;
        if (helper) {
            hip_check(hipEventRecord(fill_done_[part.region].get(), stream), "hipEventRecord");
            walk_stream = trace_stream_.get();
            hip_check(hipStreamWaitEvent(walk_stream, fill_done_[part.region].get(), 0), "hipStreamWaitEvent");
            if (chain) hip_check(hipMemsetAsync(d_rows, 0, (size_t)n * 2 * AL, walk_stream), "hipMemsetAsync(rows)");
            if (chain && chain->min_start) {
                hip_check(hipMemsetD32Async((hipDeviceptr_t)chain->min_start, AL, 1, walk_stream), "hipMemsetD32Async(first column)");
                t.min_start = chain->min_start;
            }
        }
        hip_check(hipLaunchKernel((const void *)&traceback_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256),
                                  targs, 0, walk_stream),
                  "hipLaunchKernel(traceback_kernel)");
        if (chain && chain->min_start && chain->packed) {
            CompactArgs c{t.rows, chain->packed, chain->min_start, 2 * cnt, AL};
            void *cargs[] = {&c};
            hip_check(hipLaunchKernel((const void *)&compact_rows_kernel, dim3((unsigned)(2 * cnt)), dim3(256), cargs, 0, walk_stream),
                      "hipLaunchKernel(compact_rows_kernel)");
        }
        // records (and ops) of the part, behind its walk and before the part's end cells and region are reused
        if (cigar_) launch_cigar(walk_stream, t.rows, t.idx, part_ends, begin, cnt);
        if (helper) {
            hip_check(hipEventRecord(trace_done_[part.region].get(), walk_stream), "hipEventRecord");
            region_used[part.region] = true;
        }
    }
    if (chain) {                                       // the walk is the caller's to wait for (trace_done(region))
        chain_regions_busy_[chain->region] = true;
        return true;
    }
    if (helper)                                        // the call stays asynchronous on `stream`: it ends when the walks have
        for (int r = 0; r < 2; ++r)
            if (region_used[r]) hip_check(hipStreamWaitEvent(stream, trace_done_[r].get(), 0), "hipStreamWaitEvent");
    return false;
}

void Engine::ensure_trace_stream() {
    if (trace_done_[1]) return;             // (the last one created: a failure part-way starts over)
    trace_stream_ = make_stream("traceback");
    entry_ev_ = make_event(hipEventDisableTiming);
    for (int r = 0; r < 2; ++r) {
        fill_done_[r] = make_event(hipEventDisableTiming);
        trace_done_[r] = make_event(hipEventDisableTiming);
    }
}

bool Engine::align_fused(int alg, long long n, const uint8_t *d_reads, const uint8_t *d_refs, uint8_t *d_rows, short *d_idx,
                 hipStream_t stream) {
    const FusedGeometry *best = nullptr;
    WaveLds best_lds{};
    int best_total = 0, best_blocks = 0;
    double best_cost = 0;
    for (const FusedGeometry &g : kFusedGeometries) {
        if (g.G * g.K < R_) continue;
        const WaveLds w = g.lds(R_, F_);
        const int blocks8 = (F_ + g.G - 1 + 7) / 8;
        const int total = g.total(w.total, R_, F_, blocks8);
        if (total > kMaxBlockLds - 8192) continue;
        const double cost = (double)(F_ + g.G - 1) * (g.K * 9.0 + 7.0);         // single-wave latency
        if (!best || cost < best_cost) {
            best = &g;
            best_lds = w;
            best_total = total;
            best_blocks = blocks8;
            best_cost = cost;
        }
    }
    if (!best) return false;
    FillArgs f{};
    put_sweep(f, d_reads, d_refs, n, best_blocks, best_lds);
    f.out_rows = d_rows;
    f.out_idx = d_idx;
    if (cigar_) {                          // the end cells leave the wave's LDS too: the encoder places the alignment with them
        if (sizeof(EndCell) * (size_t)n > d_ends_.bytes()) {
            hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
            if (trace_stream_) hip_check(hipStreamSynchronize(trace_stream_.get()), "hipStreamSynchronize");
            d_ends_.reserve(sizeof(EndCell) * (size_t)n, "end cells");
        }
        f.ends = d_ends_.get();
    }
    const void *fn = best->kernel[alg];
    ran_align_fill_ = ran_fill_name(AlignRoute::Fused);
    ran_align_geo_ = nullptr;
    ran_result_format_ = cigar_ ? "cigar" : "rows";
    align_ptr_bytes_per_pair_ = (long long)best->G * best_blocks * best->K * 4 / 2;
    if (best_total > kDefaultBlockLds)
        hip_check(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, best_total),
                  "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    const long long ppw = 2 * (kWave / best->G);
    void *fargs[] = {&f};
    hip_check(hipLaunchKernel(fn, dim3((unsigned)((n + ppw - 1) / ppw)), dim3(kWave), fargs, (size_t)best_total, stream),
              "hipLaunchKernel(align_fill_tag_kernel, fused)");
    if (cigar_) launch_cigar(stream, d_rows, d_idx, d_ends_.get(), 0, n);
    return true;
}

// what the two walks' TraceArgs share (register sweep: G x K is the geometry; strips: 64 x K and the padding of all strips)
TraceArgs Engine::trace_args(int alg, const uint8_t *d_reads, const uint8_t *d_refs, long long n, const unsigned *ptr, const EndCell *ends,
                             uint8_t *rows, short *idx, int G, int K, int pad_rows, int blocks8) const {
    TraceArgs t{};
    put_sweep(t, d_reads, d_refs, n, blocks8);
    t.ptr = ptr;
    t.ends = ends;
    t.rows = rows;
    t.idx = idx;
    t.G = G;
    t.K = K;
    t.pad_rows = pad_rows;
    t.alg = alg;
    t.affine = sc_.affine ? 1 : 0;
    t.sse_policy = sse_policy_ ? 1 : 0;
    return t;
}

void Engine::align_strips_device(const StripMode &mode, long long n, const uint8_t *d_reads, const uint8_t *d_refs, uint8_t *d_rows,
                         short *d_idx, hipStream_t stream) {
    // ---- the plan (strip_plan.h): rows per lane, strips, what a pair-of-pairs holds in the scratch, the chunk ----
    const int K = strip_rows_per_lane(R_, mode, strip_k_);
    if (!K) throw std::runtime_error("no strip alignment kernel for this mode");
    const StripGeometry &geo = *std::find_if(std::begin(kStripGeometries), std::end(kStripGeometries), [&](const StripGeometry &g) { return g.K == K; });
    const WaveLds &lds = geo.lds;
    BandShape band = kNoBand;           // every strip's pointer region is sized by the widest strip window (the block band, band_window.h)
    if (mode.band) {
        int block_rows, col_align;
        band_block_shape(block_rows, col_align);
        band = strip_band_shape(R_, band_width_, block_rows, col_align);
    }
    const StripPlan plan = strip_plan(R_, F_, K, mode, band);
    const int strips = plan.strips, AL = R_ + F_;
    align_ptr_bytes_per_pair_ = plan.ptr_bytes_per_pair;
    align_ckpt_bytes_per_pair_ = plan.ckpt_bytes_per_pair;
    size_t free_b = 0, total_b = 0;
    hip_check(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
    const long long chunk = strip_chunk_pairs(strip_scratch_cap(free_b + d_ptr_.bytes(), scratch_cap_mb_), plan.bytes_per_pp, n);
    const long long waves = chunk / 2;
    // ---- reserve ----
    ensure_trace_scratch(chunk, plan.bytes_per_pp, 2, stream);      // (chunk is even: waves * bytes_per_pp bytes, chunk end cells)
    if ((size_t)2 * n * sizeof(int) > d_first_bad_.bytes()) {
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
        d_first_bad_.reserve((size_t)2 * n * sizeof(int), "first invalid positions");
    }
    WalkState *walk = mode.ckpt ? reinterpret_cast<WalkState *>(d_ptr_.get() + plan.walk_at(waves)) : nullptr;
    const void *fn = geo.kernel(mode, 0), *refill_fn = mode.ckpt ? geo.kernel(mode, 1) : fn;
    for (const void *f : {fn, refill_fn}) raise_block_lds(f, lds.total);
    // ---- launches: the rows zeroed and the first invalid positions once, then chunk after chunk its strips and its walk ----
    hip_check(hipMemsetAsync(d_rows, 0, (size_t)n * 2 * AL, stream), "hipMemsetAsync(rows)");
    hipLaunchKernelGGL(first_invalid_kernel, dim3((unsigned)n), dim3(kWave), 0, stream, d_reads, d_refs, n, R_, F_, d_first_bad_.get(),
                       sse_policy_ ? 1 : 0);
    hip_check(hipGetLastError(), "hipLaunchKernel(first_invalid_kernel)");
    for (long long begin = 0; begin < n; begin += chunk) {
        const long long cnt = std::min(chunk, n - begin), cnt_waves = (cnt + 1) / 2;
        const uint8_t *reads = d_reads + (size_t)begin * R_, *refs = d_refs + (size_t)begin * F_;
        const unsigned walk_blocks = (unsigned)((cnt + 255) / 256);
        auto launch_strip = [&](const void *kernel, int s, const char *what) {
            StripArgs a = strip_args(reads, refs, cnt, plan, lds, s, d_ptr_.get(), plan.top_at(waves, s), plan.bottom_at(waves, s), plan.f_rows_at(waves),
                                     d_ends_.get(), d_first_bad_.get() + 2 * begin);
            a.ptr = d_ptr_.get() + plan.region_at(cnt_waves, s);
            a.walk = walk;
            void *kargs[] = {&a};
            hip_check(hipLaunchKernel(kernel, dim3((unsigned)cnt_waves), dim3(kWave), kargs, (size_t)lds.total, stream), what);
        };
        for (int s = 0; s < strips; ++s) launch_strip(fn, s, "hipLaunchKernel(align_strip_kernel)");
        TraceArgs t = trace_args(mode.alg, reads, refs, cnt, d_ptr_.get(), d_ends_.get(), d_rows + (size_t)begin * 2 * AL, d_idx + (size_t)begin * 4, 64, K,
                                 plan.pad_total, plan.blocks8);
        t.strip_rows = plan.rows;
        t.strip_words = (long long)plan.region_stride(cnt_waves);
        t.wide_score = mode.wide ? 1 : 0;
        t.band = plan.band;
        if (mode.ckpt) {
            // the backward pass: per strip, last to first, re-fill it into the one region and let the walks cross it
            hipLaunchKernelGGL(walk_init_kernel, dim3(walk_blocks), dim3(256), 0, stream, (const EndCell *)d_ends_.get(), walk, cnt, AL);
            hip_check(hipGetLastError(), "hipLaunchKernel(walk_init_kernel)");
            for (int s : ckpt_rounds(strips)) {
                launch_strip(refill_fn, s, "hipLaunchKernel(align_strip_kernel, re-fill)");
                hipLaunchKernelGGL(traceback_ckpt_kernel, dim3(walk_blocks), dim3(256), 0, stream, t, walk, s);
                hip_check(hipGetLastError(), "hipLaunchKernel(traceback_ckpt_kernel)");
            }
        } else {
            void *targs[] = {&t};
            hip_check(hipLaunchKernel(mode.band ? (const void *)&traceback_band_kernel : (const void *)&traceback_kernel, dim3(walk_blocks), dim3(256), targs, 0,
                                      stream),
                      "hipLaunchKernel(traceback_kernel)");
        }
        if (cigar_) launch_cigar(stream, t.rows, t.idx, d_ends_.get(), begin, cnt);      // (before the next chunk's fill reuses d_ends_)
    }
}

// Placed scores of reads that take the row strips (Engine::score_placed_strips, engine_placed.hip): the forward pass of the
// checkpointed traceback at the K the strip rule picks, with a first-invalid table (zeros: read by the NW variant only).
Engine::PlacedSweep Engine::placed_strip_sweep(PlacedRec *d_placed) const {
    const StripMode mode{kAlgSW, sc_.affine, false, false, false, true};
    const int K = strip_rows_per_lane(R_, mode, strip_k_);
    if (!K) throw std::runtime_error("no strip kernel for placed scores");
    const StripGeometry &geo = *std::find_if(std::begin(kStripGeometries), std::end(kStripGeometries), [&](const StripGeometry &g) { return g.K == K; });
    return PlacedSweep{geo.kernel(mode, 0), geo.lds, strip_plan(R_, F_, K, mode, kNoBand), true, "placed-score boundary rows",
                       "hipLaunchKernel(align_strip_kernel, placed scores)", placed_records_step(d_placed, false)};
}

template <typename Sink>
void Engine::align_host(int opt, int n, const char *const *reads, const char *const *refs, Sink alignments,
                int threads) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ran_align_fill_ = "none";
    ran_align_geo_ = nullptr;
    ran_result_format_ = "rows";            // (before the refusals: a refused call must not report the format of an earlier one)
    const int AL = R_ + F_;
    const size_t per_pair = (size_t)3 * AL + 8;
    // (row strips run chunk after chunk on one pointer scratch: chunks that fill the device -- 2 000 pairs-of-pairs and more --
    // instead of 128 MB of staging, which is 1 100 of them at 10 kbp x 10 kbp: 253 -> ~190 ms per 4 096 pairs through the ABI)
    const RouteFacts facts = route_facts(true);
    const AlignRoute route = valign::align_route(rule_inputs(), alg, facts);       // (of a direct call; refusals leave here)
    const bool by_strips = strip_chunks(route, facts);
    const size_t chunk_bytes = by_strips && !dbg_.on("align_chunk_bytes") ? std::max<size_t>(align_chunk_bytes_, 384u << 20) : align_chunk_bytes_;
    long long chunk = per_pair ? (long long)(chunk_bytes / per_pair) : n;
    chunk = whole_rounds(chunk);
    chunk = std::max<long long>(chunk, 1024);
    chunk = std::min<long long>(chunk, n);
    reset_pipeline();
    ensure_staging(chunk);
    ensure_align_staging(chunk);
    if (threads < 1) threads = 1;
    threads = std::min(threads, 64);
    hipStream_t kernels = streams_[0].get(), copy_in = streams_[1].get(), copy_out = streams_[2].get();
    host_stats_ = HostStats{};
    if (direct_call(n, (size_t)AL)) {
        // Small call: one stream, no events.  The kernels read the sequences out of the pinned staging; rows
        // and coordinates land next to each other in one device buffer and come back in ONE copy (scattered
        // 4-byte stores over PCIe would cost a bus transaction each).
        auto t0 = std::chrono::steady_clock::now();
        uint8_t *h_reads = h_reads_[0].get(), *h_refs = h_refs_[0].get(), *h_rows = h_rows_[0].get(), *d_rows = d_rows_[0].get();
        gather(reads, refs, n, h_reads, h_refs, threads);
        auto t1 = std::chrono::steady_clock::now();
        const size_t rows_bytes = ((size_t)n * 2 * AL + 15) / 16 * 16, all_bytes = rows_bytes + sizeof(short) * 4 * (size_t)n;
        if (route == AlignRoute::Fused && align_fused(alg, n, dev_view(h_reads), dev_view(h_refs), dev_view(h_rows), (short *)(dev_view(h_rows) + rows_bytes), kernels)) {
            // ONE launch: the wave that fills a pair's pointers (kept in LDS) walks it back and writes the rows
            // straight into the pinned staging
            hip_check(hipStreamSynchronize(kernels), "hipStreamSynchronize");
            auto t2 = std::chrono::steady_clock::now();
            scatter(alignments, n, h_rows, (const short *)(h_rows + rows_bytes), threads);
            host_stats_.gather_ms = ms_between(t0, t1);
            host_stats_.wait_ms = ms_between(t1, t2);
            host_stats_.drain_ms = ms_between(t2, std::chrono::steady_clock::now());
            host_stats_.direct = 2;
            return;
        }
        // rows and coordinates sit next to each other in the slot's row buffer (it has room for both) and come
        // back in ONE copy
        short *d_idx = (short *)(d_rows + rows_bytes);
        align_device(opt, n, dev_view(h_reads), dev_view(h_refs), d_rows, d_idx, kernels);
        hip_check(hipMemcpyAsync(h_rows, d_rows, all_bytes, hipMemcpyDeviceToHost, kernels), "D2H rows + idx");
        hip_check(hipStreamSynchronize(kernels), "hipStreamSynchronize");
        auto t2 = std::chrono::steady_clock::now();
        scatter(alignments, n, h_rows, (const short *)(h_rows + rows_bytes), threads);
        host_stats_.gather_ms = ms_between(t0, t1);
        host_stats_.wait_ms = ms_between(t1, t2);
        host_stats_.drain_ms = ms_between(t2, std::chrono::steady_clock::now());
        host_stats_.direct = 1;
        return;
    }
    // A flat destination in page-locked memory (valign_hip_host_register) IS the device layout: the copy engine
    // writes the caller's buffers directly and the host has nothing left to scatter.
    uint8_t *direct_rows = nullptr;
    short *direct_idx = nullptr;
    if (!no_direct_out_) flat_destination(alignments, n, direct_rows, direct_idx);
    host_stats_.direct_out = direct_rows ? 1 : 0;
    // Result rows are right-justified strings behind zeros: on the staged paths only the columns from the chunk's smallest
    // readStart on cross PCIe, packed on the device (compact_rows_kernel; 0.42 instead of 1.36 GB per million pairs of
    // 150 x 500) -- the scatter unpacks them and writes the zeros in front, as it always did.  A registered flat
    // destination still receives whole rows straight from the copy engine: there the zeros would be the host's to write.
    auto drain = [&](int s) {
        if (slot_pending_[s] <= 0) return;
        const auto t0 = std::chrono::steady_clock::now();
        if (!direct_rows) scatter(alignments + slot_begin_[s], slot_pending_[s], h_rows_[s].get(), h_idx_[s].get(), threads, (size_t)start_col_[s]);
        host_stats_.drain_ms += ms_between(t0, std::chrono::steady_clock::now());
        host_stats_.d2h_row_bytes += (double)slot_pending_[s] * 2 * (AL - start_col_[s]);
        host_stats_.full_row_bytes += (double)slot_pending_[s] * 2 * AL;
        slot_pending_[s] = 0;
    };
    int slot = 0;
    long long chunk_no = 0;
    chain_regions_busy_[0] = chain_regions_busy_[1] = false;       // (every earlier call ended with its walks waited for)
    prime_copy_engines(copy_in, copy_out, chunk);
    if (!copy_issuer_) copy_issuer_.reset(new CopyIssuer(device_));
    CopyIssuer *copy_issuer = copy_issuer_.get();
    // An error in the middle of the pipeline must not leave copies in flight into the CALLER's buffers (registered
    // result buffers receive them directly): quiesce the issuer and the streams before the exception leaves.
    struct Quiesce {
        Engine *e;
        bool armed = true;
        ~Quiesce() {
            if (!armed) return;
            if (e->copy_issuer_) {
                try {
                    e->copy_issuer_->wait_idle();
                } catch (...) {
                }
            }
            if (e->trace_stream_) (void)hipStreamSynchronize(e->trace_stream_.get());
            for (int s = 0; s < kSlots; ++s) (void)hipStreamSynchronize(e->streams_[s].get());
            for (int s = 0; s < kSlots; ++s) e->slot_pending_[s] = 0;
        }
    } quiesce{this};
    for (long long begin = 0; begin < n; begin += chunk, slot = (slot + 1) % kSlots) {
        const long long cnt = std::min<long long>(chunk, n - begin);
        auto t0 = std::chrono::steady_clock::now();
        copy_issuer->wait_issued(slot);             // (only then is the slot's event the one of its last chunk)
        hip_check(hipEventSynchronize(slot_done_[slot].get()), "hipEventSynchronize");   // its last chunk is back on the host
        host_stats_.wait_ms += ms_between(t0, std::chrono::steady_clock::now());
        drain(slot);
        uint8_t *h_reads = h_reads_[slot].get(), *h_refs = h_refs_[slot].get(), *d_reads = d_reads_[slot].get(), *d_refs = d_refs_[slot].get();
        t0 = std::chrono::steady_clock::now();
        gather(reads + begin, refs + begin, cnt, h_reads, h_refs, threads);
        host_stats_.gather_ms += ms_between(t0, std::chrono::steady_clock::now());
        hip_check(hipMemcpyAsync(d_reads, h_reads, (size_t)cnt * R_, hipMemcpyHostToDevice, copy_in), "H2D reads");
        hip_check(hipMemcpyAsync(d_refs, h_refs, (size_t)cnt * F_, hipMemcpyHostToDevice, copy_in), "H2D refs");
        hip_check(hipEventRecord(in_done_[slot].get(), copy_in), "hipEventRecord");
        hip_check(hipStreamWaitEvent(kernels, in_done_[slot].get(), 0), "hipStreamWaitEvent");
        // the walk of this chunk runs on the helper stream beside the fill of the next one (two scratch regions)
        const bool packed = !direct_rows && !whole_rows_;
        const WalkChain chain{(int)(chunk_no & 1), chunk, packed ? d_min_start_.get() + slot : nullptr, packed ? d_packed_rows_[slot].get() : nullptr};
        const bool chained = align_device(opt, cnt, d_reads, d_refs, d_rows_[slot].get(), d_idx_[slot].get(), kernels, &chain);
        hip_check(hipEventRecord(kernels_done_[slot].get(), chained ? trace_stream_.get() : kernels), "hipEventRecord");      // the chunk's last kernel
        ++chunk_no;
        uint8_t *rows_to = direct_rows ? direct_rows + (size_t)begin * 2 * AL : h_rows_[slot].get();
        short *idx_to = direct_idx ? direct_idx + 4 * begin : h_idx_[slot].get();
        // SDMA, not a blit kernel beside the next fill: the copies are issued once the host has seen the kernels end
        CopyIssuer::Job job{kernels_done_[slot].get(), {rows_to, idx_to}, {d_rows_[slot].get(), d_idx_[slot].get()},
                            {(size_t)cnt * 2 * AL, sizeof(short) * 4 * (size_t)cnt}, copy_out, slot_done_[slot].get(), slot};
        start_col_[slot] = 0;
        if (chained && packed) {        // (the stream-order fallback -- row strips, a scratch too small for two regions -- copies whole rows)
            job.src[0] = d_packed_rows_[slot].get();
            job.d_min = d_min_start_.get() + slot;
            job.h_min = h_min_start_.get() + slot;
            job.row_bytes = AL;
            job.rows = 2 * cnt;
            job.col = &start_col_[slot];
        }
        copy_issuer->submit(job);
        slot_begin_[slot] = begin;
        slot_pending_[slot] = cnt;
    }
    for (int k = 0; k < kSlots; ++k) {              // oldest chunk first
        const int s = (slot + k) % kSlots;
        const auto t0 = std::chrono::steady_clock::now();
        copy_issuer->wait_issued(s);
        hip_check(hipEventSynchronize(slot_done_[s].get()), "hipEventSynchronize");
        host_stats_.wait_ms += ms_between(t0, std::chrono::steady_clock::now());
        drain(s);
    }
    quiesce.armed = false;               // (everything has been waited for)
}

void Engine::prime_copy_engines(hipStream_t copy_in, hipStream_t copy_out, long long staged_pairs) {
    if (copy_engines_primed_) return;
    copy_engines_primed_ = true;
    const size_t in_bytes = std::min<size_t>((size_t)staged_pairs * F_, 128u << 20);
    const size_t out_bytes = std::min<size_t>(sizeof(short) * 4 * (size_t)staged_pairs, 4096);
    if (in_bytes < (16u << 20) || out_bytes == 0) return;         // (too short to still be running when the second copy is issued)
    hip_check(hipStreamSynchronize(copy_in), "hipStreamSynchronize");
    hip_check(hipStreamSynchronize(copy_out), "hipStreamSynchronize");
    hip_check(hipMemcpyAsync(d_refs_[0].get(), h_refs_[0].get(), in_bytes, hipMemcpyHostToDevice, copy_in), "H2D (engine priming)");
    // the input copy must have reached its engine before the result stream asks which engines are free: >= 16 MB
    // take >= 0.3 ms on the wire, a tenth of that is plenty for the submission
    for (const auto t0 = std::chrono::steady_clock::now(); ms_between(t0, std::chrono::steady_clock::now()) < 0.1;) {
    }
    hip_check(hipMemcpyAsync(h_idx_[0].get(), d_idx_[0].get(), out_bytes, hipMemcpyDeviceToHost, copy_out), "D2H (engine priming)");
    hip_check(hipStreamSynchronize(copy_out), "hipStreamSynchronize");
    hip_check(hipStreamSynchronize(copy_in), "hipStreamSynchronize");
}

void Engine::ensure_trace_scratch(long long pairs, size_t bytes_per_pp, long long ppw, hipStream_t stream) {
    const long long waves = (pairs + ppw - 1) / ppw;
    const size_t need = (size_t)(waves * (ppw / 2)) * bytes_per_pp, ends = sizeof(EndCell) * (size_t)(waves * ppw);
    if (need <= d_ptr_.bytes() && ends <= d_ends_.bytes()) return;
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");   // nothing may still read the old scratch
    if (trace_stream_) hip_check(hipStreamSynchronize(trace_stream_.get()), "hipStreamSynchronize");
    chain_regions_busy_[0] = chain_regions_busy_[1] = false;
    d_ptr_.reserve(need, "pointer scratch");
    d_ends_.reserve(ends, "end cells");
}

void Engine::ensure_align_staging(long long pairs) {
    if (pairs <= align_staged_pairs_) return;
    align_staged_pairs_ = 0;
    const size_t AL = (size_t)R_ + F_;
    for (int s = 0; s < kSlots; ++s) {
        h_rows_[s].reset();
        h_idx_[s].reset();
        d_rows_[s].reset();
        d_idx_[s].reset();
        // (room for the coordinates behind the rows: small calls bring both back in one piece)
        const size_t rows_cap = (size_t)pairs * 2 * AL + sizeof(short) * 4 * (size_t)pairs + 32;
        h_rows_[s].reserve(rows_cap);
        h_idx_[s].reserve(sizeof(short) * 4 * (size_t)pairs);
        d_rows_[s].reserve(rows_cap);
        d_idx_[s].reserve(sizeof(short) * 4 * (size_t)pairs);
        d_packed_rows_[s].reserve((size_t)pairs * 2 * AL + 64, "packed rows");
    }
    d_min_start_.reserve(sizeof(int) * kSlots, "first columns");        // (fixed sizes: once)
    h_min_start_.reserve(sizeof(int) * kSlots, "first columns");
    align_staged_pairs_ = pairs;
}

// the two sinks of align_host: the ABI's Alignment array, and caller-provided contiguous buffers (valign_hip_align_host)
template void Engine::align_host<Alignment *>(int, int, const char *const *, const char *const *, Alignment *, int);
template void Engine::align_host<FlatSink>(int, int, const char *const *, const char *const *, FlatSink, int);

}  // namespace valign
