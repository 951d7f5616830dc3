// engine_core.hip -- Engine: construction, launch-plan selection, staging, describe().
#include <numeric>

#include "engine.hip.h"

namespace valign {

// The side geometry: 8 x 19, ONE kernel, the compact row-table stream's LDS; no fill, placed, suboptimal or extension kernel
static WaveLds side_tile_lds(int R, int F) { return row_table_lds16(R, F); }
static Geometry side_geometry() {
    Geometry g{kSideTileG, kSideTileK, false, &side_tile_lds, {}, {}, [](int, int) -> const void * { return nullptr; },
               [](int, int) -> const void * { return nullptr; }, [](int) -> const void * { return nullptr; }, [](int) -> const void * { return nullptr; }};
    g.kernel[kAlgSW][kGapAffineSym] = (const void *)&score_kernel<kSideTileG, kSideTileK, kAlgSW, kGapAffineSym>;
    return g;
}
const Geometry kSideGeometry = side_geometry();

Engine::Engine(int device, int R, int F, const Scoring &sc, int force_g, int force_k)
    : device_(device), R_(R), F_(F), sc_(sc) {
    if (R < 0 || F < 0) throw std::runtime_error("negative sequence length");
    if ((long long)R + F > 32767)
        throw std::runtime_error("read_length + ref_length exceeds the ABI's 16-bit coordinates");
    validate_scoring();
    int count = 0;
    hip_check(hipGetDeviceCount(&count), "hipGetDeviceCount");
    if (device < 0 || device >= count)
        throw std::runtime_error("HIP device " + std::to_string(device) + " not present (" +
                                 std::to_string(count) + " visible): libHIPKernel.so has no CPU path");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hipDeviceProp_t prop;
    hip_check(hipGetDeviceProperties(&prop, device_), "hipGetDeviceProperties");
    arch_ = prop.gcnArchName;
    cu_count_ = prop.multiProcessorCount;
    if (arch_.find("gfx950") == std::string::npos)
        throw std::runtime_error("device is " + arch_ + "; this library carries gfx950 code only");
    force_g_ = force_g;
    force_k_ = force_k;
    // The side tile is in no table: forcing it forces the SCORE launches (score_plan_for), and everything else the engine does
    // plans as an unforced engine of this shape would -- the tile has no other kernel.
    side_forced_ = tilt_tables_only(force_g, force_k);
    if (side_forced_) {
        if (R_ > kSideTileRows)
            throw std::runtime_error("the forced kernel geometry does not fit read_length=" + std::to_string(R) + ", ref_length=" + std::to_string(F));
        force_g = force_k = 0;
    }
    plan_ = choose_plan(R_, F_, force_g, force_k);
    align_resident_ = plan_;
    // Reads of more than 1 536 rows would take the 64 x 32 geometry -- 45 to 53 KB of LDS, three waves per CU --: the long-read
    // kernels (512-row strips, 12 to 15 waves per CU) sweep them 15 to 55 % faster (2 000 x 4 000: 6.2 -> 7.9 TCUPS linear,
    // 3.6 -> 5.6 affine; profiles/r04_rate_sweep.txt).  A forced geometry is a forced geometry.
    if (!force_g && !force_k && !plan_.long_mode && plan_.geo && plan_.geo->G * plan_.geo->K > 1536) plan_ = long_plan();
    // The resident kernels keep the slab numbers of the whole reference in LDS (2 ref_length bytes per lane group, and as
    // much again to stage it): at 150 x 8 000 one wave fills a CU's LDS -- 2.3 TCUPS, 0.7 at 150 x 32 000 -- where the
    // long-read kernels, whose slab numbers go through a ring, sweep 10.9 / 10.2 (affine: 1.5 / 0.4 against 5.9 / 5.6; their
    // single-strip instances, profiles/r04_rate_sweep.txt).  One wave per CU: always.  Two: with linear gaps, or when the
    // 160-row strips pad the read no worse than the resident geometry (150 x 4 000 affine: 2.9 -> 6.0).  Up to four (from about
    // 1 500 columns on): under the same padding condition (150 x 2 000: 8.7 -> 11.0 / 5.7 -> 6.0; 100 x 2 000 stays: 128 rows
    // against 160).
    if (!force_g && !force_k && !plan_.long_mode && plan_.geo) {
        const int waves_per_cu = std::min(32, (kMaxBlockLds / std::max(1, plan_.lds.total * plan_.waves_per_block)) * plan_.waves_per_block);
        const int strip_rows = kLongG * kLongK;
        // (reads of up to 1 024 rows take the 160-row strips; beyond, the 512-row ones, which the 64 x 24 geometry still beats)
        const bool pads_alike = R_ <= 1024 && ((R_ + strip_rows - 1) / strip_rows) * strip_rows * 100 <= plan_.geo->G * plan_.geo->K * 115;
        if (waves_per_cu <= 1 || (waves_per_cu <= 2 && (!sc_.affine || pads_alike)) || (waves_per_cu <= 4 && pads_alike)) plan_ = long_plan();
    }
    base_plan_ = plan_;
    latency_plan_ = (force_g || force_k || plan_.long_mode) ? plan_ : choose_plan(R_, F_, 0, 0, true);
    build_length_classes();
    for (int s = 0; s < kSlots; ++s) streams_[s] = make_stream();
    for (int s = 0; s < kSlots; ++s) {
        slot_done_[s] = make_event(hipEventDisableTiming);
        in_done_[s] = make_event(hipEventDisableTiming);
        kernels_done_[s] = make_event(hipEventDisableTiming | hipEventBlockingSync);     // (the copy issuer sleeps on it)
    }
}

// The members free the buffers, then destroy the events and streams (engine.hip.h), with this device current.
Engine::~Engine() {
    copy_issuer_.reset();               // (joins its thread; nothing is queued outside a call)
    (void)hipSetDevice(device_);
    if (trace_stream_) (void)hipStreamSynchronize(trace_stream_.get());
}

const char *Engine::score_cell_format(int alg, long long n) const {
    if (alg > 1) return "none";
    // the long-read kernels (a band takes them; int32 cells exist there only): the route's cells (long_plan.h)
    if (plan_.long_mode || band_width_ > 0 || score_wide_cells(alg)) return long_cells_name(long_mode(alg, false).cells);
    // the plan score_device launches for a call of n pairs: small calls sweep on the latency plan, whose rows enter the
    // NW variant's tilt
    const LaunchPlan &plan = (n > 0 && n <= (long long)latency_plan_.pairs_per_wave * 1024 && band_width_ == 0) ? latency_plan_ : plan_;
    return gap_form_f16(score_gap_form(rule_inputs(), alg, R_, F_, plan.geo->G * plan.geo->K)) ? "f16" : "int16";
}

std::string Engine::ran_score_cells() const {
    if (!ran_score_cells_) return "none";
    std::string s;
    for (const auto &f : {std::make_pair(kRanF16, "f16"), std::make_pair(kRanInt16, "int16"), std::make_pair(kRanInt32, "int32")})
        if (ran_score_cells_ & f.first) s += (s.empty() ? "" : "+") + std::string(f.second);
    return s;
}

std::string Engine::ran_kernels() const {
    return "{\"ran_score_cells\": \"" + ran_score_cells() + "\", \"ran_align_fill\": \"" + ran_align_fill_ + "\"}";
}

bool Engine::score_int16_ok(int alg) const {
    int rows = 0;
    if (!plan_.long_mode && plan_.geo) rows = plan_.geo->G * plan_.geo->K;
    if (latency_plan_.geo && !latency_plan_.long_mode) rows = std::max(rows, latency_plan_.geo->G * latency_plan_.geo->K);
    return int16_range_ok(rule_inputs(), alg, true, plan_.long_mode, rows);
}

std::string Engine::host_phases() const {
    char buf[320];
    snprintf(buf, sizeof buf, "{\"host_gather_ms\": %.3f, \"host_wait_ms\": %.3f, \"host_drain_ms\": %.3f, \"host_classify_ms\": %.3f, \"host_launch_ms\": %.3f, \"d2h_row_mb\": %.1f, \"full_row_mb\": %.1f}",
             host_stats_.gather_ms, host_stats_.wait_ms, host_stats_.drain_ms, host_stats_.classify_ms, host_stats_.launch_ms,
             host_stats_.d2h_row_bytes / 1e6, host_stats_.full_row_bytes / 1e6);
    return buf;
}

std::string Engine::describe(int opt, long long n) const {
    // the launch plan of a SCORE call of (opt, n): the engine's -- or the 8 x 19 side tile where score_device would take it
    // (score_plan_for and few_pairs: the decision score_device makes)
    LaunchPlan shown = plan_;
    const int alg_shown = opt & 0xF;
    if (alg_shown <= kAlgNW && !plan_.long_mode && band_width_ == 0 && !score_wide_cells(alg_shown))
        shown = score_plan_for(plan_, alg_shown, R_, F_, few_pairs(n), false);
    const long long ppb = (long long)shown.pairs_per_wave * shown.waves_per_block;
    int band_rows = 0, band_align = 0;
    band_block_shape(band_rows, band_align);
    char buf[4096];
    snprintf(buf, sizeof buf,
             "{\"arch\": \"%s\", \"device\": %d, \"alg\": %d, \"affine\": %d, \"group_lanes\": %d, "
             "\"rows_per_lane\": %d, \"padded_rows\": %d, \"pairs_per_wave\": %d, \"waves_per_block\": %d, "
             "\"lds_per_wave\": %d, \"lds_per_block\": %d, \"steps\": %d, \"blocks\": %lld, \"long_mode\": %d, "
             "\"band_width\": %d, \"ragged_batching\": %d, \"ragged_launches\": %d, \"ragged_cell_fraction\": %.4f, "
             "\"score_cells\": \"%s\", \"direct_call\": %d, \"packed_classes\": %d, \"direct_out\": %d, \"band_block_rows\": %d, \"band_col_align\": %d, \"band_waves_per_cu\": %d, \"band_lds_per_wave\": %d, \"band_cells_per_pair\": %lld, \"long_strip_rows\": %d, \"d2h_row_mb\": %.1f, \"full_row_mb\": %.1f, \"host_gather_ms\": %.3f, \"host_classify_ms\": %.3f, \"host_wait_ms\": %.3f, \"host_drain_ms\": %.3f, \"ran_score_cells\": \"%s\", \"ran_align_fill\": \"%s\", "
             "\"band_alignments\": %d, \"band_nw\": %d, \"band_placed\": %d, \"align_ptr_bytes_per_pair\": %lld, \"trace_checkpoints\": %d, "
             "\"align_ckpt_bytes_per_pair\": %lld, \"align_scratch_bytes\": %lld, \"ran_result_format\": \"%s\", "
             "\"cigar_d2h_bytes\": %lld, \"cigar_rows_scratch_bytes\": %lld, \"ran_placed\": \"%s\", \"placed_wide\": %d, \"placed_scratch_bytes\": %lld, "
             "\"ran_span\": \"%s\", \"span_ref_length\": %lld, \"span_scratch_bytes\": %lld, "
             "\"ran_span_cigar\": \"%s\", \"span_cigar_scratch_bytes\": %lld, "
             "\"ran_subopt\": \"%s\", \"subopt_scratch_bytes\": %lld, \"subopt_ring_cols\": %d, \"ran_extend\": \"%s\", \"extend_wide\": %d, \"extend_band\": %d, \"extend_band_block_rows\": %d, "
             "\"ran_score_geometry\": \"%s\", \"ran_align_geometry\": \"%s\", "
             "\"ran_placed_geometry\": \"%s\", \"ran_subopt_geometry\": \"%s\", \"ran_extend_geometry\": \"%s\"}",
             arch_.c_str(), device_, opt & 0xF, sc_.affine ? 1 : 0, shown.geo->G, shown.geo->K,
             shown.geo->G * shown.geo->K, shown.pairs_per_wave, shown.waves_per_block, shown.lds.total,
             shown.lds.total * shown.waves_per_block, F_ + shown.geo->G - 1, n > 0 ? (n + ppb - 1) / ppb : 0,
             plan_.long_mode ? 1 : 0, band_width_, ragged_, host_stats_.launches,
             host_stats_.cells_padded > 0 ? host_stats_.cells_swept / host_stats_.cells_padded : 1.0,
             score_cell_format(opt & 0xF, n), host_stats_.direct, host_stats_.packed, host_stats_.direct_out,
             ((opt & 0xF) == kAlgSW || band_nw_) ? band_rows : VALIGN_HIP_BAND_BLOCK_ROWS, ((opt & 0xF) == kAlgSW || band_nw_) ? band_align : VALIGN_HIP_BAND_COL_ALIGN,
             band_blocks_per_cu_, band_lds_, (band_tables_width_ == band_width_ && band_plan_.usable) ? band_plan_.cells : 0ll, long_strip_rows_, host_stats_.d2h_row_bytes / 1e6, host_stats_.full_row_bytes / 1e6, host_stats_.gather_ms, host_stats_.classify_ms, host_stats_.wait_ms,
             host_stats_.drain_ms, ran_score_cells().c_str(), ran_align_fill_, band_alignments(), band_nw(), band_placed(), align_ptr_bytes_per_pair_, trace_checkpoints(),
             align_ckpt_bytes_per_pair_, (long long)d_ptr_.bytes(), ran_result_format_, cigar_d2h_bytes_,
             (long long)(d_cig_rows_[0].bytes() + d_cig_rows_[1].bytes()), ran_placed_, placed_wide(), (long long)(d_placed_rows_.bytes() + d_placed_ends_.bytes()),
             ran_span_.c_str(), span_ref_length(rule_inputs()), (long long)span_[kSlots].bytes(),
             ran_span_cigar_.c_str(), (long long)(span_cigar_[0].bytes() + span_cigar_[1].bytes()),
             ran_subopt_, (long long)subopt_[kSlots].bytes(), subopt_ring_cols_, ran_extend_, extend_wide(), extend_band(), VALIGN_HIP_EXTEND_BAND_BLOCK_ROWS,
             ran_geometry(ran_score_geo_).c_str(), ran_geometry(ran_align_geo_).c_str(),
             ran_geometry(ran_placed_geo_).c_str(), ran_geometry(ran_subopt_geo_).c_str(), ran_geometry(ran_extend_geo_).c_str());
    std::string out(buf);
    // extension alignments (engine_extend_align.hip): what the last call ran, on which geometry, and the pointer scratch it shares
    out.insert(out.size() - 1, std::string(", \"ran_extend_align\": \"") + ran_extend_align_ + "\", \"ran_extend_align_geometry\": \"" +
                                   ran_geometry(ran_extend_align_geo_) + "\", \"extend_align_scratch_bytes\": " +
                                   std::to_string((long long)(d_ptr_.bytes() + d_ends_.bytes() + d_extend_align_recs_.bytes())) +
                                   ", \"extend_band_align\": " + std::to_string(extend_band_align()) + ", \"ran_extend_align_chunks\": " +
                                   std::to_string(ran_extend_align_chunks_) + ", \"ran_cigar_lanes\": " + std::to_string(ran_cigar_lanes_));
    // the Z-drop of extension calls (engine_extend.hip): the key, the Z the last extension call ran under, the waves that skipped a strip in it
    out.insert(out.size() - 1, ", \"extend_zdrop\": " + std::to_string(extend_zdrop()) + ", \"ran_extend_zdrop\": " + std::to_string(ran_extend_zdrop_) +
                                   ", \"extend_zdrop_skipped_waves\": " + std::to_string(extend_zdrop_skipped_waves()) +
                                   ", \"extend_zdrop_rows\": " + std::to_string(extend_zdrop_rows()));
    if (ran_score_sym_affine_)         // only where the last score call ran the int16 symmetric affine SW kernel
        out.insert(out.size() - 1, std::string(", \"ran_score_sym_affine\": \"") + ran_score_sym_affine_ + "\", \"ran_score_sym_affine_frame\": \"" +
                                       ran_score_sym_affine_frame_ + "\", \"ran_score_sym_affine_scores\": \"" + ran_score_sym_affine_scores_ + "\"");
    // ... and, where its last such launch ran on the 8 x 19 side tile, which form of the row-table step its waves took
    if (ran_score_sym_affine_ && ran_score_geo_ == &kSideGeometry)
        out.insert(out.size() - 1, std::string(", \"ran_score_sym_affine_form\": \"") + ran_side_tile_form() + "\"");
    return out;
}

void Engine::band_block_shape(int &block_rows, int &col_align) const {
    const bool chain = long_mode(kAlgSW, false).chain;       // (of a Smith-Waterman call: describe() names the API's blocks for a refused NW one)
    block_rows = chain ? kBandK : VALIGN_HIP_BAND_BLOCK_ROWS;
    col_align = chain ? VALIGN_HIP_BAND_CHAIN_COL_ALIGN : VALIGN_HIP_BAND_COL_ALIGN;
}

void Engine::validate_scoring() {
    auto fits = [](int v) { return v >= -32768 && v <= 32767; };
    if (!fits(sc_.match) || !fits(sc_.mismatch) || !fits(sc_.gap_read) || !fits(sc_.gap_ref) ||
        !fits(sc_.open_read) || !fits(sc_.ext_read) || !fits(sc_.open_ref) || !fits(sc_.ext_ref))
        throw std::runtime_error("scoring parameter outside int16");
    // The row padding and the unsigned floor-at-zero arithmetic need non-positive gap scores.
    const bool gaps_ok = sc_.affine ? (sc_.open_read <= 0 && sc_.ext_read <= 0 && sc_.open_ref <= 0 && sc_.ext_ref <= 0)
                                    : (sc_.gap_read <= 0 && sc_.gap_ref <= 0);
    if (!gaps_ok) throw std::runtime_error("positive gap scores are not supported by the HIP kernels");
    // Affine model: a maximal run of k gap bases costs open + (k - 1) * extend.  The Gotoh recurrence only
    // computes that while extending is not dearer than opening -- otherwise it re-opens instead (H of the
    // previous cell may itself end in a gap), which exhaustive enumeration exposes
    // (tests/golden/make_affine_golden.py).  Refused rather than silently computing another model.
    if (sc_.affine && (sc_.ext_read < sc_.open_read || sc_.ext_ref < sc_.open_ref))
        throw std::runtime_error("affine gap scores need extend >= open in each direction (an extension dearer "
                                 "than the opening is not an affine model)");
}

LaunchPlan Engine::choose_plan(int R, int F, int force_g, int force_k, bool latency, bool full_only) const {
    LaunchPlan best;
    double best_cost = 0;
    for (int i = 0; i < kNumGeometries; ++i) {
        const Geometry &g = kGeometries[i];
        if (g.G * g.K < R) continue;
        if (full_only && !g.full) continue;
        if (force_g && (g.G != force_g || (force_k && g.K != force_k))) continue;
        if (!force_g && force_k && g.K != force_k) continue;
        LaunchPlan p;
        p.geo = &g;
        p.lds = g.lds(R, F);
        p.pairs_per_wave = 2 * (kWave / g.G);
        // Block size: 4-wave blocks put one wave on each SIMD and measured fastest whenever two
        // of them fit a CU's 160 KiB of LDS; otherwise take the size that keeps most waves resident.
        int best_waves = 0;
        if (p.lds.total * 8 <= kMaxBlockLds) {
            p.waves_per_block = 4;
            best_waves = std::min(32, (kMaxBlockLds / (p.lds.total * 4)) * 4);
        } else {
            for (int wpb = 4; wpb >= 1; wpb >>= 1) {
                if (p.lds.total * wpb > kMaxBlockLds) continue;
                const int resident = std::min(32, (kMaxBlockLds / (p.lds.total * wpb)) * wpb);
                // (a smaller block for half as many waves again or more: five one-wave blocks were slower than one block of
                // four at 150 x 2 000, 10.9 against 9.7 ms per 131 072 alignments)
                if (resident > best_waves && (best_waves == 0 || 2 * resident >= 3 * best_waves)) {
                    best_waves = resident;
                    p.waves_per_block = wpb;
                }
            }
        }
        if (best_waves == 0) continue;
        // lane-steps per pair, weighted by instructions per step: per-row work + fixed part, measured
        // on the score kernels (5.6 / 9.3 packed instructions per register, linear / affine), and a
        // penalty for long register tiles, which lose occupancy (16x12: +14 %, 16x16: +35 %,
        // 8x20: +60 % per step over the linear estimate; tools/shape_sweep.sh).  (The penalty dates from kernels bound by
        // the LDS profile and by occupancy.  The row-table path of the int16 symmetric affine SW sweep is bound by neither:
        // its 8 x 19 side tile is no entry of this table and is not costed here -- score_plan_for takes it by rule.)
        double per_step = g.K * (sc_.affine ? 9.3 : 5.6) + 7.0;
        if (g.K > 10) per_step *= 1.0 + 0.06 * (g.K - 10);
        double cost = (double)(F + g.G - 1) * per_step * g.G / 2.0;
        if (best_waves < 8) cost *= 1.0 + 0.08 * (8 - best_waves);         // fewer than two waves per SIMD
        if (latency) cost = (double)(F + g.G - 1) * (g.K * (sc_.affine ? 9.3 : 5.6) + 7.0);
        if (!best.geo || cost < best_cost) {
            best = p;
            best_cost = cost;
        }
    }
    if (!best.geo || (dbg_.on("force_long") && !force_g)) {
        if (force_g || force_k)
            throw std::runtime_error("the forced kernel geometry does not fit read_length=" + std::to_string(R) +
                                     ", ref_length=" + std::to_string(F));
        return long_plan();
    }
    return best;
}

LaunchPlan Engine::side_plan(int R, int F) {
    LaunchPlan p;
    p.geo = &kSideGeometry;
    p.lds = kSideGeometry.lds(R, F);
    p.waves_per_block = kSideTileBlockWaves;
    p.pairs_per_wave = 2 * (kWave / kSideTileG);
    return p;
}

const char *Engine::side_tile_refusal(int alg, int R, int F, bool latency) const {
    const RuleInputs in = rule_inputs();
    const int gaps = alg <= kAlgNW ? score_gap_form(in, alg, R, F, kSideTileRows) : -1;
    return sym_affine_side_tile_refusal(in, alg, gaps, R, F, latency, side_forced_);
}

const char *Engine::ran_side_tile_form() const {
    if (!d_form_seen_.get()) return "none";
    unsigned seen[2] = {0, 0};
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    hip_check(hipMemcpy(seen, d_form_seen_.get(), sizeof seen, hipMemcpyDeviceToHost), "hipMemcpy(form words)");
    return seen[0] && seen[1] ? "both" : (seen[1] ? "row_tables_repair" : (seen[0] ? "row_tables" : "none"));
}

void Engine::reset_side_tile_form(hipStream_t stream) {
    if (!d_form_seen_.get()) return;             // (allocated by the first 8 x 19 launch, zeroed there)
    if (stream) hip_check(hipMemsetAsync(d_form_seen_.get(), 0, 2 * sizeof(unsigned), stream), "hipMemsetAsync(form words)");
    else hip_check(hipMemset(d_form_seen_.get(), 0, 2 * sizeof(unsigned)), "hipMemset(form words)");
}

LaunchPlan Engine::score_plan_for(const LaunchPlan &base, int alg, int R, int F, bool latency, bool refuse) const {
    const bool chosen = (force_g_ || force_k_) && !side_forced_;         // another forced geometry is a forced geometry
    if (chosen) return base;
    const char *refusal = side_tile_refusal(alg, R, F, latency);
    if (!refusal[0]) return side_plan(R, F);
    if (side_forced_ && refuse) throw std::runtime_error(std::string("group_lanes = 8, rows_per_lane = 19: ") + refusal);
    return base;
}

LaunchPlan Engine::long_plan() {        // row strips + column phases: any length the ABI allows
    LaunchPlan p;
    p.long_mode = true;
    p.pairs_per_wave = 2 * (kWave / kLongG);
    p.waves_per_block = 1;
    p.lds.total = LongLds<kLongG, kLongK>::kTotal;
    for (int i = 0; i < kNumGeometries; ++i)
        if (kGeometries[i].G == kLongG && kGeometries[i].K == kLongK) p.geo = &kGeometries[i];
    return p;
}

long long Engine::whole_rounds(long long pairs, bool sw_scores) const {
    if (plan_.long_mode || !plan_.geo || cu_count_ <= 0) return pairs;
    const long long waves_per_cu = std::min<long long>(32, (kMaxBlockLds / std::max(1, plan_.lds.total * plan_.waves_per_block)) * plan_.waves_per_block);
    long long round_pairs = std::max<long long>(1, waves_per_cu) * cu_count_ * plan_.pairs_per_wave;
    // ... and where this engine's Smith-Waterman score calls take the 8 x 19 side tile, of that plan's rounds too (two 4-wave
    // blocks per CU, 16 pairs per wave: 32,768 pairs on 256 CUs, a multiple of the 16,384 of 16 x 10)
    if (sw_scores && !((force_g_ || force_k_) && !side_forced_) && !side_tile_refusal(kAlgSW, R_, F_, false)[0]) {
        const LaunchPlan side = side_plan(R_, F_);
        const long long side_waves = std::min<long long>(32, (kMaxBlockLds / std::max(1, side.lds.total * side.waves_per_block)) * side.waves_per_block);
        const long long side_round = std::max<long long>(1, side_waves) * cu_count_ * side.pairs_per_wave;
        round_pairs = round_pairs / std::gcd(round_pairs, side_round) * side_round;
    }
    return pairs >= round_pairs ? pairs / round_pairs * round_pairs : pairs;
}

bool Engine::direct_call(long long n, size_t per_pair) const {
    return direct_bytes_ > 0 && (size_t)n * per_pair <= direct_bytes_ && n <= staged_pairs_;
}

void Engine::reset_pipeline() {
    bool stale = false;
    for (int s = 0; s < kSlots; ++s) stale = stale || slot_pending_[s] != 0;
    if (!stale) return;
    if (copy_issuer_) {
        try {
            copy_issuer_->wait_idle();
        } catch (...) {
        }
    }
    if (trace_stream_) (void)hipStreamSynchronize(trace_stream_.get());
    for (int s = 0; s < kSlots; ++s) {
        (void)hipStreamSynchronize(streams_[s].get());
        slot_pending_[s] = 0;
        slot_begin_[s] = 0;
    }
}

void Engine::ensure_staging(long long pairs) {
    if (pairs <= staged_pairs_) return;
    staged_pairs_ = 0;
    for (int s = 0; s < kSlots; ++s) {          // (every old block goes before the first new one is allocated)
        h_reads_[s].reset();
        h_refs_[s].reset();
        h_scores_[s].reset();
        d_reads_[s].reset();
        d_refs_[s].reset();
        d_scores_[s].reset();
        d_pack_reads_[s].reset();
        d_pack_refs_[s].reset();
    }
    for (int s = 0; s < kSlots; ++s) {
        // (write-combined pinned memory for the input staging was tried: no gain -- the call is bound by the H2D
        // copies, 12-14 ms per 650 MB while the host threads gather, and by what else runs on the box)
        h_reads_[s].reserve(std::max<size_t>((size_t)pairs * R_, 16));
        h_refs_[s].reserve(std::max<size_t>((size_t)pairs * F_, 16));
        h_scores_[s].reserve(sizeof(short) * (size_t)pairs);
        d_reads_[s].reserve(std::max<size_t>((size_t)pairs * R_, 16));
        d_refs_[s].reserve(std::max<size_t>((size_t)pairs * F_, 16));
        d_scores_[s].reserve(sizeof(short) * (size_t)pairs);
        // (the 4-bit class copies of the score path; the pinned staging above is large enough for them)
        d_pack_reads_[s].reserve(std::max<size_t>((size_t)pairs * packed_length(R_), 16));
        d_pack_refs_[s].reserve(std::max<size_t>((size_t)pairs * packed_length(F_), 16));
    }
    staged_pairs_ = pairs;
}

void Engine::build_length_classes() {
    std::vector<int> caps;
    for (int i = 0; i < kNumGeometries; ++i) {
        const int rows = kGeometries[i].G * kGeometries[i].K;
        if (rows < R_) caps.push_back(rows);
    }
    caps.push_back(R_);
    std::sort(caps.begin(), caps.end());
    caps.erase(std::unique(caps.begin(), caps.end()), caps.end());
    read_caps_ = caps;
    ref_caps_.clear();
    const int width = 64 * std::max(1, (F_ + 64 * kMaxScoreGroups - 1) / (64 * kMaxScoreGroups));
    for (int c = width; c < F_; c += width) ref_caps_.push_back(c);
    ref_caps_.push_back(F_);
    read_class_.assign((size_t)R_ + 1, 0);
    for (int len = 0, c = 0; len <= R_; ++len) {
        while (read_caps_[c] < len) ++c;
        read_class_[len] = (unsigned char)c;
    }
    ref_class_.assign((size_t)F_ + 1, 0);
    for (int len = 0, c = 0; len <= F_; ++len) {
        while (ref_caps_[c] < len) ++c;
        ref_class_[len] = (unsigned short)c;
    }
    // debug switches (VALIGN_HIP_DEBUG): small bins / chunks so that tests reach the pipeline's corners at test sizes
    ragged_min_ = std::max(1ll, dbg_.value("ragged_min", ragged_min_));
    score_chunk_bytes_ = (size_t)std::max(4096ll, dbg_.value("chunk_bytes", (long long)score_chunk_bytes_));
    align_chunk_bytes_ = (size_t)std::max(4096ll, dbg_.value("align_chunk_bytes", (long long)align_chunk_bytes_));
    direct_bytes_ = (size_t)std::max(0ll, dbg_.value("direct_bytes", (long long)direct_bytes_));
}

const LaunchPlan &Engine::class_plan(int R, int F) {
    const std::pair<int, int> key(R, F);
    auto it = class_plans_.find(key);
    if (it == class_plans_.end()) it = class_plans_.emplace(key, choose_plan(R, F, 0, 0)).first;
    return it->second;
}

int Engine::trimmed_length(const unsigned char *s, int len) {
    static const struct Table {
        bool acgt[256] = {};
        Table() { for (const char *p = "ACGTacgt"; *p; ++p) acgt[(unsigned char)*p] = true; }
    } table;
    while (len >= 8) {                      // NUL padding, eight bytes at a time
        uint64_t tail;
        memcpy(&tail, s + len - 8, 8);
        if (tail != 0) break;
        len -= 8;
    }
    while (len > 0 && !table.acgt[s[len - 1]]) --len;
    return len;
}

}  // namespace valign
