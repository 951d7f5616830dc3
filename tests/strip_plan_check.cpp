// strip_plan_check.cpp -- the plan of the row-strip alignment path (versalignlib_amd/csrc/strip_plan.h) on the CPU: the
// availability matrix, the rows-per-lane rule, every field of the plan against the arithmetic restated here, the layout of the
// scratch, and ckpt_plan.h as a view of it.  Plain g++, no HIP (tests/test_strip_plan.py builds and runs it;
// tools/sanitize.sh runs it under ASan + UBSan).
#include <stdio.h>

#include <string>
#include <utility>
#include <vector>

#include "ckpt_plan.h"
#include "strip_plan.h"

using namespace valign;

namespace {

int failures = 0;
void expect(bool ok, const std::string &what) {
    if (ok) return;
    if (++failures <= 20) fprintf(stderr, "FAIL: %s\n", what.c_str());
}

const int Ks[] = {8, 12, 16};

StripMode mode_of(int alg, bool affine, bool sse, bool wide, bool band, bool ckpt) {
    StripMode m;
    m.alg = alg;
    m.affine = affine;
    m.sse = sse;
    m.wide = wide;
    m.band = band;
    m.ckpt = ckpt;
    return m;
}
std::string name(const StripMode &m) {
    return std::string(m.alg == kAlgSW ? "SW" : "NW") + (m.affine ? " affine" : "") + (m.sse ? " sse" : "") + (m.wide ? " int32" : "") + (m.band ? " band" : "") +
           (m.ckpt ? " ckpt" : "");
}
std::vector<StripMode> all_modes() {          // every combination of the six fields, existing or not
    std::vector<StripMode> v;
    for (int bits = 0; bits < 64; ++bits) v.push_back(mode_of(bits & 1, bits & 2, bits & 4, bits & 8, bits & 16, bits & 32));
    return v;
}

// ---- 1. what is compiled, as the issue lists it ----
bool listed(int K, const StripMode &m) {
    if (m.ckpt) return !m.sse && !m.wide && !m.band;                                           // checkpointed: both gap models, every K
    if (m.band) return !m.sse && (m.wide ? K == 8 : (K == 16 || K == 8));                      // band: int16 at 16 and 8, int32 at 8, none at 12
    if (m.affine && m.sse) return false;                                                       // (the SSE kernels have linear gaps only)
    if (m.wide) return K == 8 || (m.alg == kAlgNW && !m.affine && !m.sse);                     // int32: all at 8, NW linear default at 16 / 12
    return true;                                                                               // plain, affine, SSE: every K
}

void check_matrix() {
    int existing = 0;
    for (const StripMode &m : all_modes()) {
        for (int K : Ks) {
            expect(strip_instance_exists(K, m) == listed(K, m), "availability: K " + std::to_string(K) + ", " + name(m));
            existing += strip_instance_exists(K, m) ? 1 : 0;
        }
        for (int K : {0, 4, 10, 24, 32}) expect(!strip_instance_exists(K, m), "no such rows per lane: " + std::to_string(K));
    }
    // 18 plain / affine / SSE, 12 checkpointed modes (two passes each: 24 kernels), 8 int32, 8 + 4 banded
    expect(existing == 18 + 12 + 8 + 12, "modes that exist: " + std::to_string(existing));
    static_assert(strip_instance_exists(16, StripMode{}) && !strip_instance_exists(12, StripMode{kAlgSW, false, false, false, true, false}), "constexpr");
}

// ---- 2. rows per lane: the cost rule at its edges ----
void check_rows_per_lane() {
    const StripMode plain = mode_of(kAlgSW, false, false, false, false, false), band = mode_of(kAlgSW, false, false, false, true, false);
    const StripMode wide_sw = mode_of(kAlgSW, false, false, true, false, false), wide_nw = mode_of(kAlgNW, false, false, true, false, false);
    expect(strip_rows_per_lane(1025, plain, 0) == 12, "1025 rows, every K: two strips of 768");
    expect(strip_rows_per_lane(1025, mode_of(kAlgNW, true, false, false, false, true), 0) == 12, "1025 rows, checkpointed affine");
    expect(strip_rows_per_lane(1025, band, 0) == 8, "1025 rows under a band: no 12");
    expect(strip_rows_per_lane(1025, wide_sw, 0) == 8, "1025 rows, int32 SW: 8 only");
    expect(strip_rows_per_lane(1025, wide_nw, 0) == 12, "1025 rows, int32 NW linear: every K");
    expect(strip_rows_per_lane(1024, plain, 0) == 16 && strip_rows_per_lane(2048, plain, 0) == 16, "whole strips of 1024");
    expect(strip_rows_per_lane(1, plain, 0) == 8 && strip_rows_per_lane(512, plain, 0) == 8 && strip_rows_per_lane(513, plain, 0) == 12, "short reads pad least");
    expect(strip_rows_per_lane(10000, plain, 0) == 16, "10 kbp");
    for (int K : Ks) {
        expect(strip_rows_per_lane(1025, plain, K) == K && strip_rows_per_lane(3000, plain, K) == K, "forced_k honoured");
        expect(strip_rows_per_lane(1025, band, K) == (K == 12 ? 0 : K), "forced_k under a band");
        expect(strip_rows_per_lane(1025, wide_sw, K) == (K == 8 ? K : 0), "forced_k on int32 SW");
    }
    expect(strip_rows_per_lane(1025, plain, 10) == 0 && strip_rows_per_lane(1025, mode_of(kAlgSW, true, true, false, false, false), 0) == 0, "none");
    // the rule, restated: cost = padded rows x {1.0, 1.115, 1.147}, the first of 16, 12, 8 wins a tie
    for (const StripMode &m : all_modes())
        for (int R : {1, 511, 512, 513, 768, 769, 1024, 1025, 1536, 1537, 2048, 2049, 3072, 3073, 10000, 32000}) {
            int want = 0;
            double want_cost = 0;
            for (int K : {16, 12, 8}) {
                if (!listed(K, m)) continue;
                const long long padded = (long long)((R + 64 * K - 1) / (64 * K)) * 64 * K;
                const double cost = padded * (K == 16 ? 1.0 : K == 12 ? 1.115 : 1.147);
                if (!want || cost < want_cost) want = K, want_cost = cost;
            }
            expect(strip_rows_per_lane(R, m, 0) == want, "rows per lane at " + std::to_string(R) + ", " + name(m));
        }
}

// ---- 3. the plan's fields against their arithmetic, restated; the layout ----
// the band window of one row (include/valign_hip.h has the definition): columns [lo, hi]
void row_window(int row, int R, int F, int w, int B, int A, long long &lo, long long &hi) {
    const int pad = (R + B - 1) / B * B - R;
    const int blk = (row + pad) / B;
    const long long r_lo = std::max(0, blk * B - pad), r_hi = std::min(R - 1, blk * B - pad + B - 1);
    lo = std::max(0ll, r_lo * F / R - w);
    lo -= lo % A;
    hi = std::min<long long>(F - 1, r_hi * F / R + w);
}

struct Span {
    size_t lo, hi;      // dwords [lo, hi)
    std::string what;
};

void check_layout(const StripPlan &p, const StripMode &m, long long waves, long long cnt_waves, const std::string &at) {
    std::vector<Span> spans;
    const size_t row = (size_t)waves * p.row_dwords;
    for (int s = 0; s < (m.ckpt ? 1 : p.strips); ++s)
        spans.push_back(Span{p.region_at(cnt_waves, s), p.region_at(cnt_waves, s) + (size_t)cnt_waves * p.strip_words, "region " + std::to_string(s)});
    // the row sets that are written: below every strip but the last
    std::vector<size_t> sets;
    for (int s = 0; s + 1 < p.strips; ++s) {
        const size_t b = p.bottom_at(waves, s);
        expect(p.top_at(waves, s + 1) == b, "the row set below strip s is the top of strip s + 1: " + at);
        if (s > 0) expect(p.top_at(waves, s) != b, "a strip reads and writes different row sets: " + at);
        bool seen = false;
        for (size_t o : sets) seen = seen || o == b;
        if (m.ckpt) expect(!seen, "every checkpoint is kept: " + at);
        else expect(b == p.bottom_at(waves, s & 1), "two sets ping-pong: " + at);
        if (!seen) sets.push_back(b);
    }
    expect(p.f_rows_at(waves) == row, "the F rows lie one row of every wave behind the H rows: " + at);
    for (size_t b : sets)
        for (int k = 0; k < p.row_sets; ++k) spans.push_back(Span{b + k * row, b + (k + 1) * row, "row set"});
    if (m.ckpt) spans.push_back(Span{p.walk_at(waves), p.walk_at(waves) + (size_t)(2 * waves * kWalkStateBytes + 3) / 4, "walk states"});
    const size_t total = (size_t)waves * p.bytes_per_pp;
    for (size_t i = 0; i < spans.size(); ++i) {
        expect(spans[i].lo < spans[i].hi && spans[i].hi * 4 <= total, spans[i].what + " inside the scratch: " + at);
        for (size_t j = i + 1; j < spans.size(); ++j)
            expect(spans[i].hi <= spans[j].lo || spans[j].hi <= spans[i].lo, spans[i].what + " and " + spans[j].what + " overlap: " + at);
    }
    expect(p.region_stride(cnt_waves) == (size_t)cnt_waves * p.strip_words && p.boundary_at(waves) % 64 == 0, "strides: " + at);
}

void check_plans() {
    const int Rs[] = {1, 511, 512, 513, 768, 769, 1024, 1025, 1536, 1537, 2049, 10000};
    const int Fs[] = {1, 57, 58, 64, 200, 4100};
    const int widths[] = {2, 64, 1000};
    const std::pair<int, int> shapes[] = {{VALIGN_HIP_BAND_BLOCK_ROWS, VALIGN_HIP_BAND_COL_ALIGN}, {VALIGN_HIP_BAND_CHAIN_BLOCK_ROWS, VALIGN_HIP_BAND_CHAIN_COL_ALIGN}};
    long long plans = 0, banded = 0;
    for (const StripMode &m : all_modes())
        for (int K : Ks) {
            if (!strip_instance_exists(K, m)) continue;
            for (int R : Rs)
                for (int F : Fs)
                    for (int wi = 0; wi < (m.band ? 3 : 1); ++wi)
                        for (int si = 0; si < (m.band ? 2 : 1); ++si) {
                            const int width = widths[wi], B = shapes[si].first, A = shapes[si].second;
                            const BandShape bs = m.band ? strip_band_shape(R, width, B, A) : kNoBand;
                            const StripPlan p = strip_plan(R, F, K, m, bs);
                            const std::string at = std::to_string(R) + " x " + std::to_string(F) + ", K " + std::to_string(K) + ", " + name(m) +
                                                   (m.band ? ", band " + std::to_string(width) + " on blocks of " + std::to_string(B) : "");
                            ++plans;
                            const long long rows = 64ll * K, S = std::max(1ll, (R + rows - 1) / rows), pad = S * rows - R;
                            expect(p.rows == rows && p.strips == S && p.pad_total == pad && pad >= 0 && pad < rows, "strips: " + at);
                            // the widest strip window: each strip's rows from its first real row's window start to its last row's window end
                            long long max_cols = F;
                            if (m.band) {
                                ++banded;
                                expect(bs.half == width / 2 && bs.block_rows == B && bs.col_align == A && bs.pad == (R + B - 1) / B * B - R, "band shape: " + at);
                                max_cols = 0;
                                for (long long s = 0; s < S; ++s) {
                                    long long lo, hi, lo2, hi2;
                                    row_window((int)std::max(0ll, s * rows - pad), R, F, width / 2, B, A, lo, hi);
                                    row_window((int)((s + 1) * rows - pad - 1), R, F, width / 2, B, A, lo2, hi2);
                                    max_cols = std::max(max_cols, hi2 - lo + 1);
                                }
                                expect(max_cols >= 1 && max_cols <= F, "a window lies inside the matrix: " + at);
                            }
                            expect(p.max_cols == max_cols, "widest window: " + at);
                            const long long blocks8 = (max_cols + 70) / 8, row_dwords = ((F + 71) / 64 + 2) * 64;
                            const long long strip_words = blocks8 * 64 * K * (m.affine ? 2 : 1), row_sets = (m.affine ? 2 : 1) * (m.wide ? 2 : 1);
                            expect(p.blocks8 == blocks8 && p.row_dwords == row_dwords && (long long)p.strip_words == strip_words && p.row_sets == row_sets, "sizes: " + at);
                            expect(p.blocks8 * 8 >= max_cols + 63 && p.row_dwords % 64 == 0 && p.row_dwords >= F + 135 - 64, "a sweep fits its blocks and rows: " + at);
                            const long long full = 4 * strip_words * S + 8 * row_sets * row_dwords;
                            const long long ckpt = 4 * strip_words + (S - 1) * row_sets * row_dwords * 4 + 2 * kWalkStateBytes;
                            expect((long long)p.bytes_per_pp == (m.ckpt ? ckpt : full), "bytes per pair-of-pairs: " + at);
                            expect(p.ptr_bytes_per_pair == 4 * strip_words * (m.ckpt ? 1 : S) / 2, "align_ptr_bytes_per_pair: " + at);
                            expect(p.ckpt_bytes_per_pair == (m.ckpt ? ((S - 1) * row_sets * row_dwords * 4 + 2 * kWalkStateBytes) / 2 : 0), "align_ckpt_bytes_per_pair: " + at);
                            expect(p.band.half == bs.half && p.band.block_rows == bs.block_rows && p.band.col_align == bs.col_align && p.band.pad == bs.pad, "the band travels: " + at);
                            // a scratch for 1, 2 and 7 waves; a last chunk that is shorter
                            for (long long waves : {1ll, 2ll, 7ll})
                                for (long long cnt_waves : {waves, (waves + 1) / 2}) check_layout(p, m, waves, cnt_waves, at);
                            // ckpt_plan.h is this plan under its own names
                            if (m.ckpt) {
                                const CkptPlan c = ckpt_plan(R, F, K, m.affine);
                                expect(c.rows == p.rows && c.strips == p.strips && c.pad_total == p.pad_total && c.blocks8 == p.blocks8 && c.row_dwords == p.row_dwords &&
                                           c.row_sets == p.row_sets && c.region_bytes == p.strip_words * 4 && c.row_bytes == p.row_bytes && c.state_bytes == p.state_bytes &&
                                           c.bytes_per_pp == p.bytes_per_pp && c.full_bytes == p.strip_words * 4 * p.strips,
                                       "ckpt_plan equals strip_plan: " + at);
                                StripMode fullm = m;
                                fullm.ckpt = false;
                                expect(c.full_bytes == (size_t)2 * strip_plan(R, F, K, fullm, kNoBand).ptr_bytes_per_pair, "ckpt_plan's full-pointer figure: " + at);
                            }
                        }
        }
    expect(plans > 5000 && banded > 2000, "every case reached");
    // a mode without a band ignores the shape it is handed
    const StripPlan a = strip_plan(3000, 4100, 16, StripMode{}, strip_band_shape(3000, 64, 160, 4)), b = strip_plan(3000, 4100, 16, StripMode{}, kNoBand);
    expect(a.max_cols == 4100 && a.bytes_per_pp == b.bytes_per_pp && a.band.half < 0, "no band, no window");
}

// ---- 4. the scratch cap; the one decoding of the route ----
void check_cap_and_mode() {
    const size_t MiB = 1ull << 20, GiB = 1ull << 30;
    expect(strip_scratch_cap(0, 0) == 256 * MiB && strip_scratch_cap(511 * MiB, 0) == 256 * MiB, "at least 256 MiB");
    expect(strip_scratch_cap(100 * GiB, 0) == 50 * GiB && strip_scratch_cap(100 * GiB + 1, 0) == 50 * GiB, "half of the free memory");
    expect(strip_scratch_cap(256 * GiB, 0) == 128 * GiB && strip_scratch_cap(288 * GiB, 0) == 128 * GiB, "at most 128 GiB");
    expect(strip_scratch_cap(100 * GiB, 64) == 64 * MiB && strip_scratch_cap(0, 64) == 64 * MiB, "the configured cap");
    expect(strip_scratch_cap(2 * GiB, 4096) == 1 * GiB && strip_scratch_cap(2 * GiB, -1) == 1 * GiB, "a cap above the rule changes nothing");

    RuleInputs in;
    in.R = 3000;
    in.F = 500;
    const AlignRoute routes[] = {AlignRoute::Strip, AlignRoute::StripBand, AlignRoute::StripWide, AlignRoute::StripWideBand, AlignRoute::StripCkpt};
    for (int alg = 0; alg < 2; ++alg)
        for (int affine = 0; affine < 2; ++affine)
            for (int sse = 0; sse < 2; ++sse)
                for (AlignRoute r : routes) {
                    in.sc.affine = affine != 0;
                    in.sse_policy = sse != 0;
                    bool threw = false;
                    StripMode m;
                    try {
                        m = strip_mode(r, in, alg);
                    } catch (const std::runtime_error &e) {
                        threw = std::string(e.what()).find("linear gap model only") != std::string::npos;
                    }
                    expect(threw == (affine && sse), "traceback_policy = 1 with affine gaps is refused, nothing else");
                    if (threw) continue;
                    expect(m.alg == alg && m.affine == (affine != 0) && m.sse == (sse != 0), "alg, gaps and tie-breaks of the mode");
                    expect(m.wide == (r == AlignRoute::StripWide || r == AlignRoute::StripWideBand) && m.band == (r == AlignRoute::StripBand || r == AlignRoute::StripWideBand) &&
                               m.ckpt == (r == AlignRoute::StripCkpt),
                           "cells, band and checkpoints of the route");
                }
}

}  // namespace

int main() {
    check_matrix();
    check_rows_per_lane();
    check_plans();
    check_cap_and_mode();
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("strip plan ok\n");
    return 0;
}
