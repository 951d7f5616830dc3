// engine_score.hip -- Engine: score_alignments (reference: src/Kernels/default/DefaultKernel.cpp:52-202) -- the register-sweep
// launches, the host-pointer chunk pipeline, 4-bit class unpacking and length-sorted batches.  The pipeline's pieces
// (host_chunk_pairs, stage_chunk, wait_slot) and record_pipeline, the pipeline of the placed and spanned host calls, are defined
// here.  The non-template kernels of pack_kernels.hip.h / ragged_kernels.hip.h are defined in this translation unit.
#define VALIGN_TU_SCORE 1
#include "engine.hip.h"

namespace valign {

void Engine::score_device(int opt, long long n, const uint8_t *d_reads, const uint8_t *d_refs,
                  int16_t *d_scores, hipStream_t stream, bool length_sorted) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;          // reference: unsupported mode is a silent no-op
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (length_sorted) {            // (a call of its own, or score_host's direct one)
        host_stats_ = HostStats{};
        ran_score_cells_ = 0;
        ran_score_geo_ = nullptr;
        ran_score_sym_affine_ = nullptr;
        reset_side_tile_form(stream);
    }
    if (score_width_ == 16 && !score_int16_ok(alg))
        throw std::runtime_error("shape x scoring can leave the int16 range of the DP cells (read_length " +
                                 std::to_string(R_) + ", ref_length " + std::to_string(F_) + ")");
    const bool wide = score_wide_cells(alg);
    if (side_forced_ && (plan_.long_mode || wide || band_width_ > 0))
        throw std::runtime_error("group_lanes = 8, rows_per_lane = 19: the call takes the long-read kernels (a band, int32 cells, or a reference too long for the register sweep)");
    if (plan_.long_mode || wide) {      // int32 cells exist on the strip path only
        score_long_device(alg, n, d_reads, d_refs, d_scores, stream);
        return;
    }
    // ragged_batching on a device-resident batch: classify, pack and sweep by length class (ragged_kernels.hip.h).  The
    // call then WAITS for the classification (the host lays the groups out); mode 1 sweeps the batch as it stands when
    // the length classes would not skip a third of the cells.
    if (length_sorted && ragged_applies(alg) && ragged_fits(n) && n >= 2 * ragged_min_) {
        // One context (pinned histogram / tables, counters, packed buffers) serves the device-resident calls of this
        // engine: a call on ANOTHER stream than the last one first waits, on the host, until that one's kernels and
        // table copies are through -- otherwise it would rewrite the pinned tables under them.  Calls on one stream are
        // ordered by the stream.
        if (ragged_dev_done_ && ragged_dev_stream_ != stream)
            hip_check(hipEventSynchronize(ragged_dev_done_.get()), "hipEventSynchronize(previous length-sorted call)");
        if (!ragged_dev_done_) ragged_dev_done_ = make_event(hipEventDisableTiming);
        ragged_dev_stream_ = stream;
        ragged_begin(kSlots, n, d_reads, d_refs, stream);           // (a context of its own: the pipeline's slots may be busy on the engine's streams)
        const bool swept = ragged_finish(kSlots, alg, n, d_scores, stream, ragged_ == 2);
        hip_check(hipEventRecord(ragged_dev_done_.get(), stream), "hipEventRecord");
        if (swept) return;
    }
    // a batch that leaves most SIMDs with at most one wave is over when its slowest wave is: shortest sweep
    const bool few = few_pairs(n);
    launch_score(score_plan_for(few ? latency_plan_ : plan_, alg, R_, F_, few), alg, R_, F_, n, d_reads, d_refs, d_scores, stream);
}

void Engine::launch_score(const LaunchPlan &plan, int alg, int R, int F, long long n, const uint8_t *d_reads,
                  const uint8_t *d_refs, int16_t *d_scores, hipStream_t stream,
                  const LengthGroup *groups, int n_groups) {
    ScoreArgs a;
    a.reads = d_reads;
    a.refs = d_refs;
    a.scores = d_scores;
    a.n = n;
    a.R = R;
    a.F = F;
    a.n_groups = n_groups;
    a.form_seen = nullptr;
    const long long pairs_per_block = (long long)plan.pairs_per_wave * plan.waves_per_block;
    long long blocks = (n + pairs_per_block - 1) / pairs_per_block;
    if (n_groups > 0) {
        if (n_groups > kMaxScoreGroups) throw std::runtime_error("too many length groups for one launch");
        blocks = 0;
        for (int g = 0; g < n_groups; ++g) {
            blocks += (groups[g].pairs + pairs_per_block - 1) / pairs_per_block;
            if (blocks > 0x7FFFFFFFll) throw std::runtime_error("batch too large for one launch");
            a.groups[g].block_end = (unsigned)blocks;
            a.groups[g].F = groups[g].F;
            a.groups[g].n = groups[g].pairs;
            a.groups[g].pair_ofs = groups[g].pair_ofs;
            a.groups[g].read_ofs = (long long)groups[g].read_ofs;
            a.groups[g].ref_ofs = (long long)groups[g].ref_ofs;
        }
    }
    a.prof_area = plan.lds.prof_area;
    a.refc_stride = plan.lds.refc_stride;
    a.wave_lds = plan.lds.total;
    put_scoring(a);
    const int gaps = score_gap_form(rule_inputs(), alg, R, F, plan.geo->G * plan.geo->K);
    const void *fn = plan.geo->kernel[alg][gaps];
    if (!fn) throw std::runtime_error("no score kernel of this gap form on " + ran_geometry(plan.geo));      // (the side geometry has one)
    ran_score_cells_ |= gap_form_f16(gaps) ? kRanF16 : kRanInt16;
    ran_score_geo_ = plan.geo;
    // int16 symmetric affine Smith-Waterman: the biased three-operand-maximum form inside its window, else gap sources.  Asked
    // about the engine's shape, which holds every launch of a length-sorted call: one form per call.
    // (the member shares its place with the linear model's gap scores, which no affine kernel reads: written for this kernel only)
    if (alg == kAlgSW && gaps == kGapAffineSym) {
        const bool max3 = sym_affine_max3_ok(rule_inputs(), R_, F_);
        a.sym_max3_bias = max3 ? sym_affine_bias(sc_) : 0;
        // ... and inside the biased form's window the tilted frame where its own, narrower window holds on this geometry (bit 16
        // of the same member says so to the kernel, which then folds 2x into its query profile)
        const bool tilted = sym_affine_tilt_ok(rule_inputs(), R_, F_, plan.geo->G * plan.geo->K, plan.geo->K);
        if (tilted) a.sym_max3_bias = sym_affine_tilt_bias(sc_) | 1 << 16;
        // ... and in the tilted frame the substitution scores from row tables in registers where every one of them is a byte (bit
        // 17): that set-up builds no profile and lays the wave's LDS out its own way, never larger than the plan's
        // (the 8 x 19 side tile runs nothing else: its plan's LDS IS the tables', with the compact stream)
        const WaveLds tables_lds = tilt_tables_only(plan.geo->G, plan.geo->K) ? plan.lds : row_table_lds(plan.geo->G, R, F);
        const bool row_tables = tilted && sym_affine_row_tables_ok(rule_inputs(), R_, F_, plan.geo->G * plan.geo->K, plan.geo->K, plan.lds.total, tables_lds.total);
        // (that tile's kernel runs nothing else and would write no score: score_plan_for hands it out only where this holds)
        if (tilt_tables_only(plan.geo->G, plan.geo->K)) {
            if (!row_tables) throw std::runtime_error("the 8 x 19 side tile was planned for a launch whose row tables are refused");
            if (!d_form_seen_.get()) {
                d_form_seen_.reserve(2 * sizeof(unsigned), "side tile form words");
                hip_check(hipMemset(d_form_seen_.get(), 0, 2 * sizeof(unsigned)), "hipMemset(form words)");      // (once per engine, before any launch reads the pointer)
            }
            a.form_seen = d_form_seen_.get();
        }
        if (row_tables) {
            a.sym_max3_bias |= 1 << 17;
            a.prof_area = tables_lds.prof_area;
            a.refc_stride = tables_lds.refc_stride;
            a.wave_lds = tables_lds.total;
        }
        ran_score_sym_affine_ = ran_sym_affine_name(max3);
        ran_score_sym_affine_frame_ = ran_sym_affine_frame_name(tilted);
        ran_score_sym_affine_scores_ = ran_sym_affine_scores_name(row_tables);
    }
    const int block_lds = a.wave_lds * plan.waves_per_block;
    if (block_lds > kDefaultBlockLds)
        hip_check(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, block_lds),
                  "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    if (blocks > 0x7FFFFFFFll) throw std::runtime_error("batch too large for one launch");
    if (blocks == 0) return;
    void *kargs[] = {&a};
    hip_check(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(plan.waves_per_block * kWave), kargs,
                              (size_t)block_lds, stream),
              "hipLaunchKernel(score_kernel)");
}

void Engine::launch_unpack(const uint8_t *d_packed, uint8_t *d_out, long long n, int len, hipStream_t stream) {
    if (n <= 0 || len <= 0) return;
    UnpackArgs a{d_packed, d_out, n, len};
    void *kargs[] = {&a};
    const bool even = (len & 1) == 0;
    const long long items = even ? (n * (long long)(len / 2) + 7) / 8 : n * (long long)((len + 1) / 2);
    const long long blocks = (items + 255) / 256;
    if (blocks > 0x7FFFFFFFll) throw std::runtime_error("batch too large for one launch");
    hip_check(hipLaunchKernel(even ? (const void *)&unpack_even_kernel : (const void *)&unpack_odd_kernel, dim3((unsigned)blocks),
                              dim3(256), kargs, 0, stream),
              "hipLaunchKernel(unpack_kernel)");
}

long long Engine::host_chunk_pairs(bool shared_scratch, long long n, bool sw_scores) const {
    const size_t per_pair = (size_t)R_ + F_;
    const size_t chunk_bytes = shared_scratch && !dbg_.on("chunk_bytes") ? std::max<size_t>(score_chunk_bytes_, 192u << 20) : score_chunk_bytes_;
    long long chunk = per_pair ? (long long)(chunk_bytes / per_pair) : n;
    chunk = whole_rounds(chunk, sw_scores);
    chunk = std::max<long long>(chunk, 1024);
    return std::min<long long>(chunk, n);
}

void Engine::stage_chunk(int slot, hipStream_t st, const char *const *reads, const char *const *refs, long long cnt, int threads) {
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t *h_reads = h_reads_[slot].get(), *h_refs = h_refs_[slot].get(), *d_reads = d_reads_[slot].get(), *d_refs = d_refs_[slot].get();
    if (pack_) {
        // two base classes per byte across PCIe, expanded in HBM to the canonical byte of each class
        const size_t PR = packed_length(R_), PF = packed_length(F_);
        packer_.gather_packed(reads, refs, cnt, h_reads, h_refs, threads);
        host_stats_.gather_ms += ms_between(t0, std::chrono::steady_clock::now());
        hip_check(hipMemcpyAsync(d_pack_reads_[slot].get(), h_reads, (size_t)cnt * PR, hipMemcpyHostToDevice, st), "H2D reads (classes)");
        hip_check(hipMemcpyAsync(d_pack_refs_[slot].get(), h_refs, (size_t)cnt * PF, hipMemcpyHostToDevice, st), "H2D refs (classes)");
        launch_unpack(d_pack_reads_[slot].get(), d_reads, cnt, R_, st);
        launch_unpack(d_pack_refs_[slot].get(), d_refs, cnt, F_, st);
        host_stats_.packed = 1;
    } else {
        gather(reads, refs, cnt, h_reads, h_refs, threads);
        host_stats_.gather_ms += ms_between(t0, std::chrono::steady_clock::now());
        hip_check(hipMemcpyAsync(d_reads, h_reads, (size_t)cnt * R_, hipMemcpyHostToDevice, st), "H2D reads");
        hip_check(hipMemcpyAsync(d_refs, h_refs, (size_t)cnt * F_, hipMemcpyHostToDevice, st), "H2D refs");
    }
}

void Engine::wait_slot(int slot, const std::function<void(int)> &drain) {
    const auto t0 = std::chrono::steady_clock::now();
    hip_check(hipEventSynchronize(slot_done_[slot].get()), "hipEventSynchronize");
    const auto t1 = std::chrono::steady_clock::now();
    drain(slot);
    host_stats_.wait_ms += ms_between(t0, t1);
    host_stats_.drain_ms += ms_between(t1, std::chrono::steady_clock::now());
}

void Engine::ensure_record_staging(long long pairs, const RecordKind &kind) {
    const size_t bytes = kind.bytes * (size_t)pairs;
    if (bytes <= record_staged_bytes_) return;
    record_staged_bytes_ = 0;
    for (int s = 0; s < kSlots; ++s) {          // (every old block goes before the first new one is allocated)
        h_records_[s].reset();
        d_records_[s].reset();
    }
    for (int s = 0; s < kSlots; ++s) {
        h_records_[s].reserve(bytes);
        d_records_[s].reserve(bytes, kind.label);
    }
    record_staged_bytes_ = bytes;
}

void Engine::record_pipeline(long long n, const char *const *reads, const char *const *refs, void *out, const RecordKind &kind, long long chunk,
                             bool one_stream, int threads, const ChunkLaunch &launch) {
    const size_t per_pair = (size_t)R_ + F_;
    reset_pipeline();
    ensure_staging(chunk);
    ensure_record_staging(chunk, kind);
    threads = std::min(std::max(threads, 1), 64);
    host_stats_ = HostStats{};
    if (direct_call(n, per_pair)) {
        // small call: the kernels read the gathered sequences out of the pinned staging and write their records there
        auto t0 = std::chrono::steady_clock::now();
        gather(reads, refs, n, h_reads_[0].get(), h_refs_[0].get(), threads);
        auto t1 = std::chrono::steady_clock::now();
        launch(0, n, dev_view(h_reads_[0].get()), dev_view(h_refs_[0].get()), dev_view(h_records_[0].get()), streams_[0].get());
        hip_check(hipStreamSynchronize(streams_[0].get()), "hipStreamSynchronize");
        auto t2 = std::chrono::steady_clock::now();
        memcpy(out, h_records_[0].get(), kind.bytes * (size_t)n);
        host_stats_.gather_ms = ms_between(t0, t1);
        host_stats_.wait_ms = ms_between(t1, t2);
        host_stats_.drain_ms = ms_between(t2, std::chrono::steady_clock::now());
        host_stats_.direct = 1;
        return;
    }
    const std::function<void(int)> drain = [&](int s) {
        if (slot_pending_[s] <= 0) return;
        memcpy((uint8_t *)out + kind.bytes * (size_t)slot_begin_[s], h_records_[s].get(), kind.bytes * (size_t)slot_pending_[s]);
        slot_pending_[s] = 0;
    };
    int slot = 0;
    for (long long begin = 0; begin < n; begin += chunk, slot = (slot + 1) % kSlots) {
        const long long cnt = std::min<long long>(chunk, n - begin);
        wait_slot(slot, drain);                 // the result of the chunk that used this slot
        hipStream_t st = streams_[one_stream ? 0 : slot].get();
        stage_chunk(slot, st, reads + begin, refs + begin, cnt, threads);
        launch(slot, cnt, d_reads_[slot].get(), d_refs_[slot].get(), d_records_[slot].get(), st);
        hip_check(hipMemcpyAsync(h_records_[slot].get(), d_records_[slot].get(), kind.bytes * (size_t)cnt, hipMemcpyDeviceToHost, st), kind.d2h);
        hip_check(hipEventRecord(slot_done_[slot].get(), st), "hipEventRecord");
        slot_begin_[slot] = begin;
        slot_pending_[slot] = cnt;
    }
    for (int k = 0; k < kSlots; ++k) wait_slot((slot + k) % kSlots, drain);          // oldest chunk first
}

void Engine::score_host(int opt, int n, const char *const *reads, const char *const *refs, short *scores,
                int threads, int16_t *d_dest) {
    const int alg = opt & 0xF;
    if (alg > 1 || n <= 0) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ran_score_cells_ = 0;
    ran_score_geo_ = nullptr;
    ran_score_sym_affine_ = nullptr;
    const size_t per_pair = (size_t)R_ + F_;
    // Long reads on row strips: their launches follow one another on one stream (the strips' boundary rows are one scratch) and
    // a 48 MB chunk of 10 kbp pairs is 1 200 waves for 3 500 resident ones -- each launch runs at a third of the device.
    // Chunks of up to 192 MB there.  The route says which calls these are (long_plan.h): what score_device sends to the long-read
    // kernels (int32 cells exist there only) and whose launches hand boundary rows on through the scratch.  The banded block
    // chain keeps nothing in HBM between its steps: its chunks may run side by side on the slots' streams -- a chunk of 2 400
    // pairs of 10 kbp fills 600 of the 4 096 resident waves and takes a launch's latency whatever its size -- and so do the
    // single-strip instances (short reads against a long reference).
    const bool shared_scratch = (plan_.long_mode || score_wide_cells(alg)) && long_mode(alg, false).brow;
    const bool strips_in_turn = plan_.long_mode && shared_scratch;
    const bool sw_scores = alg == kAlgSW;
    const long long chunk = host_chunk_pairs(strips_in_turn, n, sw_scores);
    reset_pipeline();
    reset_side_tile_form(nullptr);
    ensure_staging(chunk);
    if (threads < 1) threads = 1;
    threads = std::min(threads, 64);
    if (direct_call(n, per_pair) && (!ragged_applies(alg) || d_dest)) {      // (length-sorted batching is a property of the pipeline)
        // Small call (the reference's timing loop is 100 of them back to back, src/impl/main.cpp:278-287): what
        // it costs is API calls, not bytes.  The kernel reads the gathered sequences straight out of the pinned
        // staging over PCIe and writes its scores into pinned host memory: one launch and one wait instead of
        // three copies, a launch, an event and four event waits.
        host_stats_ = HostStats{};
        auto t0 = std::chrono::steady_clock::now();
        gather(reads, refs, n, h_reads_[0].get(), h_refs_[0].get(), threads);
        auto t1 = std::chrono::steady_clock::now();
        score_device(opt, n, dev_view(h_reads_[0].get()), dev_view(h_refs_[0].get()), d_dest ? d_dest : (int16_t *)dev_view(h_scores_[0].get()),
                     streams_[0].get());
        hip_check(hipStreamSynchronize(streams_[0].get()), "hipStreamSynchronize");
        auto t2 = std::chrono::steady_clock::now();
        if (!d_dest) memcpy(scores, h_scores_[0].get(), sizeof(short) * (size_t)n);
        host_stats_.gather_ms = ms_between(t0, t1);
        host_stats_.wait_ms = ms_between(t1, t2);
        host_stats_.drain_ms = ms_between(t2, std::chrono::steady_clock::now());
        host_stats_.direct = 1;
        return;
    }
    // length-sorted batching: the decision is the host's (a sample of the call's tails), the work the device's -- every chunk
    // is classified, packed by length class and swept class by class in HBM (ragged_kernels.hip.h)
    const bool ragged = !d_dest && ragged_applies(alg) && ragged_fits(chunk) &&
                        (ragged_ == 2 || sampled_cell_fraction(reads, refs, n) < 0.67);
    host_stats_ = HostStats{};
    const std::function<void(int)> drain = [&](int s) {
        if (slot_pending_[s] <= 0) return;
        if (d_dest) {                          // (the kernels wrote the device destination themselves)
            slot_pending_[s] = 0;
            return;
        }
        memcpy(scores + slot_begin_[s], h_scores_[s].get(), sizeof(short) * (size_t)slot_pending_[s]);
        slot_pending_[s] = 0;
    };
    // what follows a chunk's kernels: the scores' way home and the slot's event.  A length-sorted chunk gets there one
    // iteration late: its classification runs on the device while the host gathers the next chunk, and only then does
    // the host read the histogram, lay the groups out and launch the sweeps (ragged_finish) -- no wait in between.
    auto finish_chunk = [&](int s, long long pairs) {
        hipStream_t cs = streams_[shared_scratch ? 0 : s].get();
        if (ragged) (void)ragged_finish(s, alg, pairs, d_scores_[s].get(), cs, true);
        if (!d_dest)
            hip_check(hipMemcpyAsync(h_scores_[s].get(), d_scores_[s].get(), sizeof(short) * (size_t)pairs, hipMemcpyDeviceToHost, cs), "D2H scores");
        hip_check(hipEventRecord(slot_done_[s].get(), cs), "hipEventRecord");
    };
    // (two iterations late, in fact: one gather is about as long as a chunk's copy + classification, two leave room)
    struct OpenChunk {
        int slot;
        long long pairs;
    };
    std::vector<OpenChunk> open;               // length-sorted chunks whose sweeps are not launched yet, oldest first
    constexpr size_t kOpenChunks = 2;          // (< kSlots - 1: a slot comes round again only after its chunk is finished)
    int slot = 0;
    // Ramp: the device idles until the first chunk is gathered and copied, so the first chunks are short (a quarter,
    // then half a chunk); chunks of many calls deep in the pipeline stay large (fewer launches, full waves).
    long long chunk_no = 0, cnt = 0;
    for (long long begin = 0; begin < n; begin += cnt, slot = (slot + 1) % kSlots, ++chunk_no) {
        const long long ramp = (n > 2 * chunk) ? (chunk_no == 0 ? whole_rounds(chunk / 4, sw_scores) : (chunk_no == 1 ? whole_rounds(chunk / 2, sw_scores) : chunk)) : chunk;
        cnt = std::min<long long>(std::max<long long>(ramp, 1024), n - begin);
        wait_slot(slot, drain);                 // the result of the chunk that used this slot
        // kernels that share a scratch (strip boundary rows) stay on one stream
        hipStream_t st = streams_[shared_scratch ? 0 : slot].get();
        stage_chunk(slot, st, reads + begin, refs + begin, cnt, threads);
        const uint8_t *d_reads = d_reads_[slot].get(), *d_refs = d_refs_[slot].get();
        if (!ragged) {
            score_device(opt, cnt, d_reads, d_refs, d_dest ? d_dest + begin : d_scores_[slot].get(), st, false);
            finish_chunk(slot, cnt);
        } else {
            ragged_begin(slot, cnt, d_reads, d_refs, st);
            open.push_back(OpenChunk{slot, cnt});
            if (open.size() > kOpenChunks) {
                finish_chunk(open.front().slot, open.front().pairs);
                open.erase(open.begin());
            }
        }
        slot_begin_[slot] = begin;
        slot_pending_[slot] = cnt;
    }
    for (const OpenChunk &c : open) finish_chunk(c.slot, c.pairs);
    for (int k = 0; k < kSlots; ++k) wait_slot((slot + k) % kSlots, drain);          // oldest chunk first
}

bool Engine::ragged_applies(int alg) const {
    return ragged_ && alg <= kAlgNW && !plan_.long_mode && !force_g_ && !force_k_ && score_width_ != 32 &&
           R_ > 0 && F_ > 0 && score_int16_ok(alg);
}

double Engine::sampled_cell_fraction(const char *const *reads, const char *const *refs, long long n) const {
    const long long samples = std::min<long long>(n, 256);
    double swept = 0;
    for (long long k = 0; k < samples; ++k) {
        const long long i = k * n / samples;
        const int r = read_caps_[read_class_[trimmed_length((const unsigned char *)reads[i], R_)]];
        const int f = ref_caps_[ref_class_[trimmed_length((const unsigned char *)refs[i], F_)]];
        swept += (double)r * f;
    }
    return swept / ((double)samples * R_ * F_);
}

void Engine::ensure_ragged(int c, long long n) {
    RaggedCtx &x = rag_[c];
    if (!d_ref_class_.get()) {
        d_read_class_.reserve(read_class_.size(), "read classes");
        d_ref_class_.reserve(sizeof(uint16_t) * ref_class_.size(), "ref classes");
        hip_check(hipMemcpy(d_read_class_.get(), read_class_.data(), read_class_.size(), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(hipMemcpy(d_ref_class_.get(), ref_class_.data(), sizeof(uint16_t) * ref_class_.size(), hipMemcpyHostToDevice), "hipMemcpy");
    }
    if (!x.counted) x.counted = make_event(hipEventDisableTiming);
    x.counters.reserve(sizeof(unsigned) * (kRaggedMaxBins + kRaggedMaxGroups), "ragged counters");      // (fixed sizes: once)
    x.tables.reserve(kRaggedTableBytes, "ragged tables");
    x.h_counts.reserve(sizeof(unsigned) * kRaggedMaxBins);
    x.h_tables.reserve(kRaggedTableBytes);
    if (x.cap >= n) return;
    x.cap = 0;
    // (hipFree waits for the device: nothing is still reading them)
    x.reads.reset();
    x.refs.reset();
    x.scores.reset();
    x.bin.reset();
    x.pos.reset();
    x.place.reset();
    x.reads.reserve(std::max<size_t>((size_t)n * R_, 16), "ragged reads");
    x.refs.reserve(std::max<size_t>((size_t)n * F_, 16), "ragged refs");
    x.scores.reserve(sizeof(int16_t) * (size_t)n, "ragged scores");
    x.bin.reserve(sizeof(uint16_t) * (size_t)n, "ragged bins");
    x.pos.reserve(sizeof(int) * (size_t)n, "ragged places");
    x.place.reserve(sizeof(RaggedPlace) * (size_t)n, "ragged place records");
    x.cap = n;
}

void Engine::ragged_begin(int c, long long n, const uint8_t *d_reads, const uint8_t *d_refs, hipStream_t stream) {
    ensure_ragged(c, n);
    RaggedCtx &x = rag_[c];
    x.src_reads = d_reads;
    x.src_refs = d_refs;
    const int NG = ragged_bins();
    hip_check(hipMemsetAsync(x.counters.get(), 0, sizeof(unsigned) * (kRaggedMaxBins + kRaggedMaxGroups), stream), "hipMemsetAsync");
    RaggedClassifyArgs a{d_reads, d_refs, n, R_, F_, d_read_class_.get(), d_ref_class_.get(), (int)ref_caps_.size(), NG, x.bin.get(), x.counters.get()};
    void *kargs[] = {&a};
    const long long blocks = (n + kRaggedClassifyPairs - 1) / kRaggedClassifyPairs;
    hip_check(hipLaunchKernel((const void *)&ragged_classify_kernel, dim3((unsigned)blocks), dim3(256), kargs, 0, stream),
              "hipLaunchKernel(ragged_classify_kernel)");
    hip_check(hipMemcpyAsync(x.h_counts.get(), x.counters.get(), sizeof(unsigned) * (size_t)NG, hipMemcpyDeviceToHost, stream), "D2H histogram");
    hip_check(hipEventRecord(x.counted.get(), stream), "hipEventRecord");
}

std::vector<Engine::LengthGroup> Engine::fold_groups(std::vector<long long> &total, std::vector<int> &group_of_bin) const {
    const int NR = (int)read_caps_.size(), NF = (int)ref_caps_.size(), NG = NR * NF;
    std::vector<int> target((size_t)NG);
    for (int g = 0; g < NG; ++g) target[g] = g;
    const long long bin_min = std::min<long long>(ragged_min_, 256);
    for (int rc = 0; rc < NR; ++rc) {
        long long in_class = 0;
        for (int fc = 0; fc < NF; ++fc) in_class += total[rc * NF + fc];
        if (in_class == 0) continue;
        if (in_class < ragged_min_ && rc < NR - 1) {
            for (int fc = 0; fc < NF; ++fc) {
                const int g = rc * NF + fc;
                total[g + NF] += total[g];
                total[g] = 0;
                target[g] = g + NF;
            }
            continue;
        }
        for (int fc = 0; fc < NF - 1; ++fc) {
            const int g = rc * NF + fc;
            if (total[g] == 0 || total[g] >= bin_min) continue;
            total[g + 1] += total[g];
            total[g] = 0;
            target[g] = g + 1;
        }
    }
    for (int g = NG - 1; g >= 0; --g) target[g] = target[target[g]];      // targets only point forward
    std::vector<LengthGroup> groups;
    std::vector<int> group_at((size_t)NG, -1);
    long long pair_ofs = 0;
    size_t read_ofs = 0, ref_ofs = 0;
    for (int g = 0; g < NG; ++g) {
        if (total[g] == 0) continue;
        LengthGroup lg;
        lg.R = read_caps_[g / NF];
        lg.F = ref_caps_[g % NF];
        lg.pairs = total[g];
        lg.pair_ofs = pair_ofs;
        lg.read_ofs = read_ofs;
        lg.ref_ofs = ref_ofs;
        pair_ofs += lg.pairs;
        read_ofs += (size_t)lg.pairs * lg.R;
        ref_ofs += (size_t)lg.pairs * lg.F;
        group_at[g] = (int)groups.size();
        groups.push_back(lg);
    }
    group_of_bin.assign((size_t)NG, 0);
    for (int g = 0; g < NG; ++g) group_of_bin[g] = std::max(group_at[target[g]], 0);     // (an empty bin: any group, no pair asks)
    return groups;
}

bool Engine::ragged_finish(int c, int alg, long long n, int16_t *d_scores, hipStream_t stream, bool always) {
    RaggedCtx &x = rag_[c];
    const int NG = ragged_bins();
    const auto t0 = std::chrono::steady_clock::now();
    hip_check(hipEventSynchronize(x.counted.get()), "hipEventSynchronize");
    const auto t_counted = std::chrono::steady_clock::now();
    host_stats_.classify_ms += ms_between(t0, t_counted);
    std::vector<long long> total((size_t)NG);
    long long seen = 0;
    for (int g = 0; g < NG; ++g) seen += (total[g] = (long long)x.h_counts.get()[g]);
    if (seen != n) throw std::runtime_error("length classification lost pairs");
    std::vector<int> group_of_bin;
    const std::vector<LengthGroup> groups = fold_groups(total, group_of_bin);
    double swept = 0;
    for (const LengthGroup &g : groups) swept += (double)g.pairs * g.R * g.F;
    const double padded = (double)n * R_ * F_;
    if (!always && swept >= 0.67 * padded) return false;
    const int NL = (int)groups.size();
    if (NL > kRaggedMaxGroups) throw std::runtime_error("too many length groups");
    uint16_t *h_map = reinterpret_cast<uint16_t *>(x.h_tables.get());
    RaggedGroupDev *h_groups = reinterpret_cast<RaggedGroupDev *>(x.h_tables.get() + sizeof(uint16_t) * kRaggedMaxBins);
    for (int g = 0; g < NG; ++g) h_map[g] = (uint16_t)group_of_bin[g];
    for (int l = 0; l < NL; ++l)
        h_groups[l] = RaggedGroupDev{groups[l].R, groups[l].F, groups[l].pair_ofs, (long long)groups[l].read_ofs, (long long)groups[l].ref_ofs};
    hip_check(hipMemcpyAsync(x.tables.get(), x.h_tables.get(), kRaggedTableBytes, hipMemcpyHostToDevice, stream), "H2D length groups");
    RaggedPermuteArgs pa{x.src_reads, x.src_refs, n, R_, F_, x.bin.get(), reinterpret_cast<const uint16_t *>(x.tables.get()),
                         reinterpret_cast<const RaggedGroupDev *>(x.tables.get() + sizeof(uint16_t) * kRaggedMaxBins), NL,
                         x.counters.get() + kRaggedMaxBins, x.reads.get(), x.refs.get(), x.pos.get(), x.place.get()};
    void *pargs[] = {&pa};
    hip_check(hipLaunchKernel((const void *)&ragged_place_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), pargs, 0, stream),
              "hipLaunchKernel(ragged_place_kernel)");
    hip_check(hipLaunchKernel((const void *)&ragged_copy_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), pargs, 0, stream),
              "hipLaunchKernel(ragged_copy_kernel)");
    // one launch per read class: its reference-length groups ride in the kernel's group table
    for (size_t first = 0; first < groups.size();) {
        size_t end = first;
        int widest = 0;
        while (end < groups.size() && groups[end].R == groups[first].R) widest = std::max(widest, groups[end++].F);
        launch_score(score_plan_for(class_plan(groups[first].R, widest), alg, groups[first].R, widest, false), alg, groups[first].R, widest, 0,
                     x.reads.get(), x.refs.get(), x.scores.get(), stream, groups.data() + first, (int)(end - first));
        host_stats_.launches += 1;
        first = end;
    }
    RaggedUnpermuteArgs ua{x.scores.get(), x.pos.get(), d_scores, n};
    void *uargs[] = {&ua};
    hip_check(hipLaunchKernel((const void *)&ragged_unpermute_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), uargs, 0, stream),
              "hipLaunchKernel(ragged_unpermute_kernel)");
    host_stats_.cells_swept += swept;
    host_stats_.cells_padded += padded;
    host_stats_.launch_ms += ms_between(t_counted, std::chrono::steady_clock::now());
    return true;
}

}  // namespace valign
