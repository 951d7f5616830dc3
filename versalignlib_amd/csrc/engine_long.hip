// engine_long.hip -- Engine: long reads -- row strips with boundary rows through HBM (long_kernels.hip.h) and the banded
// cyclic block chain (band_kernels.hip.h); their kernel templates are instantiated in this translation unit.
#include "engine.hip.h"

namespace valign {

// The one place a long-read score kernel is instantiated: instance number I of the G x K strips (long_instance_mode) where
// long_instance_exists (long_plan.h) says it is compiled, null elsewhere; with it the LDS of a wave.
// 16 x 10: strips of 160 rows -- the blocks the strip band is defined on (include/valign_hip.h), four lane groups = eight
// pairs per wave.  64 x 8 (round 4): strips of 512 rows for UNBANDED sweeps -- less than a third of the boundary-row traffic and
// of the per-strip work, and ONE lane group per wave, so the LDS rings shrink from four sets to one (affine: 20.7 -> 14 KB
// per wave, 7 -> 11 waves per CU).  These kernels are bound by how often a wave may issue, not by latency
// (profiles/r04_band_two_chains.txt): waves per SIMD are what they lacked.
struct LongKernel {
    const void *fn;
    int lds;
};
template <int G, int K, int I>
LongKernel long_instance() {
    constexpr LongScoreMode m = long_instance_mode(G, K, I);
    if constexpr (!long_instance_exists(G, K, m)) return LongKernel{nullptr, 0};
    else
        return LongKernel{(const void *)&score_long_kernel<G, K, m.alg, m.sym, m.cells == LongCells::Int32, m.affine, m.cells == LongCells::F16, m.single, m.nw_band>,
                          LongLds<G, K, m.affine, m.single>::kTotal};
}
template <int G, int K, int... I>
LongKernel long_kernel_in(const LongScoreMode &m, std::integer_sequence<int, I...>) {
    static const LongKernel instances[] = {long_instance<G, K, I>()...};
    return instances[long_instance_index(m)];
}
template <int G, int K>
LongKernel long_kernel(const LongScoreMode &m) {
    return long_kernel_in<G, K>(m, std::make_integer_sequence<int, kLongInstances>());
}

// ... and the chain's: [affine][same scores both ways][the NW variant], each in the unit-delay and the delay-ring form
template <int I>
const void *band_instance() {
    constexpr bool UNIT = (I & 1) != 0, SYM = (I & 2) != 0, AFFINE = (I & 4) != 0, NW = (I & 8) != 0;
    if constexpr (!long_instance_exists(kBandG, kBandK, LongScoreMode{NW ? kAlgNW : kAlgSW, true, kBandG, kBandK, LongCells::Int32, AFFINE, SYM, false, NW, false})) return nullptr;
    else return (const void *)&score_band_kernel<kBandK, SYM, UNIT, AFFINE, NW>;
}
template <int... I>
const void *band_kernel_in(const LongScoreMode &m, bool unit, std::integer_sequence<int, I...>) {
    static const void *const instances[] = {band_instance<I>()...};
    return instances[unit | m.sym << 1 | m.affine << 2 | m.nw_band << 3];
}
static const void *band_kernel(const LongScoreMode &m, bool unit) { return band_kernel_in(m, unit, std::make_integer_sequence<int, 16>()); }

// ... and its PLACED form (band_placed = 1; Smith-Waterman only): [affine][same scores both ways], unit-delay and delay ring
template <int I>
const void *band_placed_instance() {
    return (const void *)&score_band_kernel<kBandK, (I & 2) != 0, (I & 1) != 0, (I & 4) != 0, false, true>;
}
template <int... I>
const void *band_placed_kernel_in(const LongScoreMode &m, bool unit, std::integer_sequence<int, I...>) {
    static const void *const instances[] = {band_placed_instance<I>()...};
    return instances[unit | m.sym << 1 | m.affine << 2];
}
static const void *band_placed_kernel(const LongScoreMode &m, bool unit) { return band_placed_kernel_in(m, unit, std::make_integer_sequence<int, 8>()); }

// The plan's tables on the device, for the band_width of the call: a width whose plan is not usable holds none
void Engine::sync_band_tables(hipStream_t stream) {
    const BandPlan &p = band_plan_;
    if (band_tables_width_ == band_width_) return;
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    d_band_blocks_.reset();
    d_band_fill_.reset();
    if (p.usable) {
        d_band_blocks_.reserve(p.blocks.size() * sizeof(BandBlock), "band blocks");
        d_band_fill_.reserve(p.fill_to.size() * sizeof(int), "band fill");
        hip_check(hipMemcpy(d_band_blocks_.get(), p.blocks.data(), p.blocks.size() * sizeof(BandBlock), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(hipMemcpy(d_band_fill_.get(), p.fill_to.data(), p.fill_to.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy");
    }
    band_tables_width_ = band_width_;       // (only once the tables are on the device)
}

void Engine::score_band_device(const LongScoreMode &mode, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int16_t *d_scores, PlacedRec *d_placed,
                               hipStream_t stream) {
    const BandPlan &p = band_plan_;
    BandArgs a{d_reads, d_refs, d_scores, d_band_blocks_.get(), d_band_fill_.get(), n, R_, F_, p.nb, p.first_block, p.pad_rows, p.d, p.ring_depth, p.code_cols};
    put_scoring(a);
    if (d_placed) a.placed = d_placed;
    if (d_placed && mode.alg != kAlgSW) throw std::runtime_error("no placed-score kernel for this mode");
    const void *fn = d_placed ? band_placed_kernel(mode, p.unit_delay) : band_kernel(mode, p.unit_delay);
    const int lds = BandLds<kBandK>::total(p.code_cols, p.ring_depth, mode.affine);
    // as many one-wave blocks as run side by side; each takes quads of pairs in turn (band_kernels.hip.h)
    int per_cu = 0;
    hip_check(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kWave, (size_t)lds), "hipOccupancyMaxActiveBlocksPerMultiprocessor");
    band_blocks_per_cu_ = per_cu;
    band_lds_ = lds;
    const long long resident = (long long)std::max(per_cu, 1) * std::max(cu_count_, 1);
    const long long blocks = std::min<long long>((n + 3) / 4, resident);
    if (blocks > 0x7FFFFFFFll) throw std::runtime_error("batch too large for one launch");
    void *kargs[] = {&a};
    hip_check(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(kWave), kargs, (size_t)lds, stream), "hipLaunchKernel(score_band_kernel)");
}

void Engine::score_long_device(int alg, long long n, const uint8_t *d_reads, const uint8_t *d_refs, int16_t *d_scores, hipStream_t stream) {
    const LongScoreMode mode = long_mode(alg, true);        // (refusals leave here)
    ran_score_cells_ |= mode.cells == LongCells::F16 ? kRanF16 : (mode.cells == LongCells::Int32 ? kRanInt32 : kRanInt16);
    if (band_width_ > 0 && !no_band_chain_) sync_band_tables(stream);
    if (mode.chain) {
        score_band_device(mode, n, d_reads, d_refs, d_scores, nullptr, stream);
        return;
    }
    const LongSizes sz = long_strip_sizes(R_, F_, n, mode);
    long_strip_rows_ = sz.rows;
    if (sz.brow_bytes > d_brow_.bytes()) {
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
        d_brow_.reserve(sz.brow_bytes, "boundary rows");
    }
    const LongKernel k = mode.G == kLongG ? long_kernel<kLongG, kLongK>(mode) : long_kernel<kLongTallG, kLongTallK>(mode);
    LongArgs a;
    a.R = R_;
    a.F = F_;
    a.strips = sz.strips;
    a.row_dwords = sz.row_dwords;
    a.band_half = band_width_ > 0 ? band_width_ / 2 : -1;
    a.brow = d_brow_.get();
    a.pp_total = sz.pp_total;
    put_scoring(a);
    for (long long begin = 0; begin < n; begin += sz.chunk) {
        const long long cnt = std::min(sz.chunk, n - begin);
        a.reads = d_reads + (size_t)begin * R_;
        a.refs = d_refs + (size_t)begin * F_;
        a.scores = d_scores + begin;
        a.n = cnt;
        void *kargs[] = {&a};
        hip_check(hipLaunchKernel(k.fn, dim3((unsigned)((cnt + sz.ppw - 1) / sz.ppw)), dim3(kWave), kargs, (size_t)k.lds, stream),
                  "hipLaunchKernel(score_long_kernel)");
    }
}

}  // namespace valign
