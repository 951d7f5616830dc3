// long_plan_check.cpp -- the plan of the long-read score path (versalignlib_amd/csrc/long_plan.h) on the CPU: the route of a call
// against the rules restated here, the compiled instances, the strip sizes, and the block chain's plan -- its invariants, the
// shapes it falls back on, and (long_plan_check --plans, shapes on stdin) its windows and period for tests/test_long_plan.py to
// compare with tools/band_schedule_model.py.  Plain g++, no HIP (tools/sanitize.sh runs it under ASan + UBSan).
#include <stdio.h>
#include <string.h>

#include <string>

#include "long_plan.h"

using namespace valign;

namespace {

int failures = 0;
void expect(bool ok, const std::string &what) {
    if (ok) return;
    if (++failures <= 20) fprintf(stderr, "FAIL: %s\n", what.c_str());
}

RuleInputs inputs(int R, int F, bool affine, bool sym, int match = 2) {
    RuleInputs in;
    in.R = R;
    in.F = F;
    in.sc.match = match;
    in.sc.affine = affine;
    if (affine) {
        in.sc.open_read = -5, in.sc.ext_read = -1, in.sc.open_ref = sym ? -5 : -4, in.sc.ext_ref = sym ? -1 : -2;
    } else {
        in.sc.gap_read = sym ? -3 : -2, in.sc.gap_ref = sym ? -3 : -4;
    }
    return in;
}

// what a call throws ("" : nothing)
std::string refusal(const RuleInputs &in, int alg, const LongFacts &f, LongScoreMode *m = nullptr) {
    try {
        const LongScoreMode got = long_score_mode(in, alg, f);
        if (m) *m = got;
    } catch (const std::runtime_error &e) {
        return e.what();
    }
    return "";
}
bool has(const std::string &s, const char *part) { return s.find(part) != std::string::npos; }

// ---- 1. the route, against the rules as the issue states them ----
void check_routes() {
    const int F = 200, band = 200;         // (the NW band connects at every R: 201 columns)
    long long cases = 0;
    for (int alg = 0; alg < 2; ++alg)
        for (int affine = 0; affine < 2; ++affine)
            for (int sym = 0; sym < 2; ++sym)
                for (int wide = 0; wide < 2; ++wide)                    // score_width 32 (or 0 on a shape that leaves int16) / 16 (or 0)
                    for (int banded = 0; banded < 2; ++banded)
                        for (int band_nw = 0; band_nw < 2; ++band_nw)
                            for (int chain = 0; chain < 3; ++chain)     // the plan is unusable / usable / usable under no_band_chain
                                for (int sw = 0; sw < 8; ++sw)          // short_strips, no_single_strip, no_f16
                                    for (int R : {1, 160, 161, 1024, 1025}) {
                                        RuleInputs in = inputs(R, F, affine, sym);
                                        in.no_f16 = (sw & 4) != 0;
                                        LongFacts f;
                                        f.band_width = banded ? band : 0;
                                        f.band_nw = band_nw;
                                        f.wide = wide;
                                        f.short_strips = (sw & 1) != 0;
                                        f.no_single_strip = (sw & 2) != 0;
                                        f.chain_usable = banded && chain > 0;
                                        f.no_band_chain = chain == 2;
                                        const std::string at = std::string(alg ? "NW" : "SW") + (affine ? " affine" : "") + (sym ? " sym" : "") + (wide ? " wide" : "") +
                                                               (banded ? " band" : "") + (band_nw ? " band_nw" : "") + " chain " + std::to_string(chain) + " switches " +
                                                               std::to_string(sw) + " R " + std::to_string(R);
                                        ++cases;
                                        LongScoreMode m;
                                        const std::string thrown = refusal(in, alg, f, &m);
                                        if (banded && alg == kAlgNW && !band_nw) {
                                            expect(thrown == "band_width applies to Smith-Waterman scores only", "the band on the NW variant needs band_nw: " + at);
                                            // describe() still predicts: the strips an unbanded-NW kernel would run, never the NW band's
                                            const LongScoreMode p = long_score_mode(in, alg, f, false);
                                            expect(!p.chain && !p.nw_band && p.cells == (wide ? LongCells::Int32 : LongCells::Int16), "prediction for a refused call: " + at);
                                            continue;
                                        }
                                        expect(thrown.empty(), "no refusal: " + at + ": " + thrown);
                                        const LongScoreMode p = long_score_mode(in, alg, f, false);
                                        expect(long_instance_index(p) == long_instance_index(m) && p.chain == m.chain && p.G == m.G && p.brow == m.brow, "refuse changes no route: " + at);
                                        expect(m.alg == alg && m.affine == (affine != 0) && m.sym == (sym != 0) && m.nw_band == (banded && alg == kAlgNW), "alg, gaps, NW band: " + at);
                                        const bool want_chain = banded && chain == 1;
                                        expect(m.chain == want_chain, "chain: " + at);
                                        if (want_chain) {
                                            expect(m.G == 32 && m.K == 16 && m.cells == LongCells::Int32 && !m.single && !m.brow, "the chain: int32 cells, no scratch: " + at);
                                        } else {
                                            const bool int32 = wide || (banded && alg == kAlgNW);
                                            const bool tall = !banded && R > 1024 && !(sw & 1);
                                            const bool single = R <= 160 && !int32 && !banded && !(sw & 2);
                                            // (2 x min(R, 200) + 6 < 1024: half floats are exact at every R here)
                                            const bool f16 = !tall && alg == kAlgSW && !affine && sym && !int32 && !banded && !(sw & 4);
                                            expect(m.G == (tall ? 64 : 16) && m.K == (tall ? 8 : 10), "geometry: " + at);
                                            expect(m.single == single && m.brow == !single, "single strip, scratch: " + at);
                                            expect(m.cells == (f16 ? LongCells::F16 : int32 ? LongCells::Int32 : LongCells::Int16), "cells: " + at);
                                        }
                                        expect(long_instance_exists(m.G, m.K, m), "the chosen instance is compiled: " + at);
                                        expect(!long_instance_exists(m.G == 16 ? 64 : 16, m.G == 16 ? 8 : 10, m) || (!m.chain && !m.single && !m.nw_band && m.cells != LongCells::F16),
                                               "only the plain instances exist at both geometries: " + at);
                                    }
    expect(cases == 2 * 2 * 2 * 2 * 2 * 2 * 3 * 8 * 5, "every case reached");
    // no_sym: the two-gap kernels always
    RuleInputs in = inputs(161, 200, false, true);
    in.no_sym = true;
    expect(!long_score_mode(in, kAlgSW, LongFacts{}).sym && long_score_mode(in, kAlgSW, LongFacts{}).cells == LongCells::Int16, "no_sym");
    expect(std::string(long_cells_name(LongCells::F16)) == "f16" && std::string(long_cells_name(LongCells::Int16)) == "int16" &&
               std::string(long_cells_name(LongCells::Int32)) == "int32", "describe()'s names");
}

// ---- the refusals at their edges; half floats on both sides of half_float_unit_exact ----
void check_edges() {
    LongFacts f;
    f.band_nw = true;
    // windows connect once 2 (band_width / 2) + 1 >= ceil(F / R): 100 x 1000 needs band_width 10
    f.band_width = 10;
    expect(refusal(inputs(100, 1000, false, true), kAlgNW, f).empty(), "band_nw at the narrowest connecting band");
    f.band_width = 9;
    const std::string narrow = refusal(inputs(100, 1000, false, true), kAlgNW, f);
    expect(has(narrow, "band_nw: band_width 9 is too narrow for read_length 100, ref_length 1000") && has(narrow, "must be at least ceil(ref_length / read_length))"),
           "band_nw below it: " + narrow);
    expect(refusal(inputs(100, 1000, false, true), kAlgSW, f).empty(), "Smith-Waterman has no such rule");
    expect(long_score_mode(inputs(100, 1000, false, true), kAlgNW, f, false).nw_band, "a prediction does not refuse");
    // int32 cells: (R + F + 2) x the largest score below 2^28; 20 002 x 13 420 is, x 13 421 is not
    f.band_width = 512;
    expect(refusal(inputs(10000, 10000, false, true, 13420), kAlgNW, f).empty(), "int32 range at its edge");
    const std::string big = refusal(inputs(10000, 10000, false, true, 13421), kAlgNW, f);
    expect(big == "shape x scoring can leave the int32 range of the DP cells (read_length 10000, ref_length 10000)", "beyond it: " + big);
    expect(refusal(inputs(10000, 10000, false, true, 13421), kAlgSW, f).empty(), "(the rule is the banded NW variant's)");
    // match 6, gaps -3: 6 min(R, F) + 12 < 1024 up to 168 rows
    const LongFacts none;
    expect(half_float_unit_exact(inputs(168, 1000, false, true, 6).sc, 168, 1000) && !half_float_unit_exact(inputs(169, 1000, false, true, 6).sc, 169, 1000), "the edge");
    expect(long_score_mode(inputs(168, 1000, false, true, 6), kAlgSW, none).cells == LongCells::F16, "half floats while they are exact");
    expect(long_score_mode(inputs(169, 1000, false, true, 6), kAlgSW, none).cells == LongCells::Int16, "int16 beyond");
    expect(long_score_mode(inputs(160, 1000, false, true, 6), kAlgSW, none).single && long_score_mode(inputs(160, 1000, false, true, 6), kAlgSW, none).cells == LongCells::F16,
           "the single-strip form of the half-float instance");
}

// ---- the compiled instances: the count the issue lists ----
void check_instances() {
    int strips160 = 0, tall = 0, chain = 0;
    for (int i = 0; i < kLongInstances; ++i) {
        const LongScoreMode a = long_instance_mode(16, 10, i), b = long_instance_mode(64, 8, i);
        expect(long_instance_index(a) == i && long_instance_index(b) == i && a.G == 16 && a.K == 10 && b.G == 64 && b.K == 8 && !a.chain, "number -> mode -> number");
        strips160 += long_instance_exists(16, 10, a) ? 1 : 0;
        tall += long_instance_exists(64, 8, b) ? 1 : 0;
        for (auto gk : {std::pair<int, int>{32, 16}, {16, 8}, {64, 10}, {64, 16}, {0, 0}}) expect(!long_instance_exists(gk.first, gk.second, a), "no such strips");
        LongScoreMode c = a;
        c.chain = true;
        chain += long_instance_exists(32, 16, c) ? 1 : 0;
        expect(!long_instance_exists(16, 10, c) && !long_instance_exists(64, 8, c), "the chain has its own geometry");
    }
    // [affine][alg][sym][int16 / int32] at each geometry; at 16 x 10 the half-float instance and its single-strip form, 8 single strips, 4 banded NW
    expect(tall == 16 && strips160 == 16 + 2 + 8 + 4, "strip instances: " + std::to_string(strips160) + " + " + std::to_string(tall));
    // [affine][sym][NW variant], each as the unit-delay and the delay-ring kernel: 16
    expect(chain == 8, "chain modes: " + std::to_string(chain));
    expect(strips160 + tall + 2 * chain == 62, "kernels in engine_long's code object");
    static_assert(long_instance_exists(16, 10, LongScoreMode{}) && !long_instance_exists(64, 8, LongScoreMode{kAlgSW, false, 64, 8, LongCells::F16, false, true, false, false, true}),
                  "constexpr");
}

// ---- the strips' sizes, restated ----
void check_sizes() {
    for (int i = 0; i < kLongInstances; ++i)
        for (int tall = 0; tall < 2; ++tall) {
            const int G = tall ? 64 : 16, K = tall ? 8 : 10;
            const LongScoreMode m = long_instance_mode(G, K, i);
            if (!long_instance_exists(G, K, m)) continue;
            for (int R : {1, 160, 161, 512, 513, 10000})
                for (int F : {1, 47, 48, 200, 10000})
                    for (long long n : {1ll, 9ll, 4096ll, 3000000ll}) {
                        const LongSizes s = long_strip_sizes(R, F, n, m);
                        const std::string at = std::to_string(R) + " x " + std::to_string(F) + ", " + std::to_string(n) + " pairs, instance " + std::to_string(i);
                        const long long rows = G * K, ppw = 2 * (64 / G), row_dwords = (F + G + 63) / 64 * 64 + 64;
                        const long long sets = (m.cells == LongCells::Int32 ? 2 : 1) * (m.affine ? 2 : 1), per_wave = ppw * row_dwords * 4 * sets;
                        expect(s.rows == rows && s.strips == std::max(1ll, (R + rows - 1) / rows) && s.ppw == ppw && s.row_dwords == row_dwords && s.row_sets == sets, "sizes: " + at);
                        expect(s.row_dwords % 64 == 0 && s.row_dwords >= F + G && (long long)s.bytes_per_wave == per_wave, "a boundary row holds the sweep: " + at);
                        const long long cap = (8ll << 30) / per_wave * ppw;
                        expect(s.chunk == std::max(ppw, std::min(cap, (n + ppw - 1) / ppw * ppw)) && s.chunk % ppw == 0 && s.waves == s.chunk / ppw, "chunk: " + at);
                        expect(s.waves * per_wave <= (8ll << 30) && (s.chunk >= n || s.chunk + ppw > cap), "at most 8 GiB of boundary rows: " + at);
                        expect(s.pp_total == s.waves * (ppw / 2) * sets && (long long)s.brow_bytes == (m.single ? 0 : s.waves * per_wave), "the scratch: " + at);
                    }
        }
}

// ---- the block chain's plan ----
const char *fallback_reason(const BandPlan &p) {            // why a plan is not usable, from what it had computed when it gave up
    if (p.usable) return "usable";
    if (p.nb == 0) return "empty";
    if (p.code_cols == 0) return "fill";
    if (p.code_cols > 2048) return "code_cols";
    return p.ring_depth > 64 ? "ring" : "lds";
}
bool power_of_two(int v) { return v > 0 && (v & (v - 1)) == 0; }

void check_plan(int R, int F, int band, bool affine, long long &usable) {
    const BandPlan p = band_chain_plan(R, F, band, affine);
    const std::string at = std::to_string(R) + " x " + std::to_string(F) + " band " + std::to_string(band) + (affine ? " affine" : "");
    expect(p.nb % kBandG == 0 && p.nb * kBandK >= R && p.pad_rows == p.nb * kBandK - R && p.pad_rows < kBandG * kBandK && p.events == p.nb + kBandG, "blocks: " + at);
    if (!p.usable) return;
    ++usable;
    int delay_max = 0;
    long long cells = 0;
    for (int b = 0; b < p.nb; ++b) {
        const BandBlock &k = p.blocks[(size_t)b];
        if (b > p.first_block) delay_max = std::max(delay_max, k.delay);
        if (b > p.first_block) expect(p.unit_delay ? k.delay == 1 : k.delay >= 2, "delays: " + at);
        if (k.lo == 0x3FFFFFFF) continue;
        const int r_lo = std::max(b * kBandK - p.pad_rows, 0), r_hi = std::min((b + 1) * kBandK - p.pad_rows - 1, R - 1);
        cells += (long long)(k.span + 1) * (r_hi - r_lo + 1);
        expect(k.lo >= 0 && k.span >= 0 && k.lo + k.span <= F - 1 && k.start < k.lo && k.lo + k.span - k.start + 1 <= p.d * kBandG, "a window lies in the matrix and in its period: " + at);
    }
    expect(p.cells == cells && cells > 0, "cells: " + at);
    expect(p.unit_delay ? p.ring_depth == 0 : (power_of_two(p.ring_depth) && p.ring_depth > delay_max && p.ring_depth <= 64), "ring depth: " + at);
    expect(power_of_two(p.code_cols) && p.code_cols >= 128 && p.code_cols <= 2048, "code_cols: " + at);
    expect((int)p.fill_to.size() == p.events + 2 && (int)p.blocks.size() == p.events + 2, "tables: " + at);
    for (int e = 0; e < (int)p.fill_to.size(); ++e)
        expect(p.fill_to[(size_t)e] <= F && p.fill_to[(size_t)e] >= 0 && (e == 0 || (p.fill_to[(size_t)e] >= p.fill_to[(size_t)e - 1] && p.fill_to[(size_t)e] - p.fill_to[(size_t)e - 1] <= 64)),
               "fill_to: " + at);
    for (int b = p.nb; b < (int)p.blocks.size(); ++b) expect(p.blocks[(size_t)b].lo == 0x3FFFFFFF && p.blocks[(size_t)b].span == 0, "an empty tail: " + at);
    expect(BandLds<kBandK>::total(p.code_cols, p.ring_depth, affine) <= 40 * 1024, "LDS: " + at);
}

void check_chain() {
    unsigned long long seed = 11;
    auto next = [&](int below) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        return 1 + (int)((seed >> 33) % (unsigned)below);
    };
    long long usable = 0, plans = 0;
    for (int i = 0; i < 300; ++i) {
        const int R = i == 0 ? 10000 : i == 1 ? 10000 : next(3000), F = i == 0 ? 10000 : i == 1 ? 5000 : next(3000);
        for (int band : {2, 16, 64, 512, 100000})
            for (int affine = 0; affine < 2; ++affine, ++plans) check_plan(R, F, band, affine, usable);
    }
    expect(usable > plans / 2, "most of the sweep is usable: " + std::to_string(usable) + " of " + std::to_string(plans));
    expect(!band_chain_plan(100, 100, 0, false).usable && band_chain_plan(100, 100, 0, false).nb == 0 && !band_chain_plan(0, 100, 8, false).usable, "no band, no plan");
    // the LDS formula is the kernel's: the query profile, two reference rings aligned to their size, the lanes' delay rings
    expect(BandLds<16>::kProfBytes == 2 * 9 * 32 * 16 && BandLds<16>::codes(512) == 9216 && BandLds<16>::codes(2048) == 10240, "profile and reference rings");
    expect(BandLds<16>::total(512, 0) == 9216 + 2 * 512 && BandLds<16>::total(512, 16) == 10240 + 64 * 16 * 4 && BandLds<16>::total(512, 16, true) == 10240 + 2 * 64 * 16 * 4,
           "unit delay: no ring; affine: two");
    // the shapes the GPU tests run (tests/test_gpu_long_plan.py): 528 x 528 has whole blocks at a slope of one -- unit delay, two
    // turns of the cycle; one row into the second turn (513) the first real block is a single row and its successor starts one
    // column on, the others sixteen: the delay ring
    expect(band_chain_plan(528, 528, 32, false).usable && band_chain_plan(528, 528, 32, true).unit_delay && band_chain_plan(528, 528, 32, false).unit_delay &&
               band_chain_plan(528, 528, 32, false).nb == 64, "528 x 528, band 32: unit delay");
    for (int F : {513, 300})
        for (int affine = 0; affine < 2; ++affine) {
            const BandPlan p = band_chain_plan(513, F, 32, affine);
            expect(p.usable && !p.unit_delay && p.ring_depth >= 4 && p.nb == 64, "513 x " + std::to_string(F) + ", band 32: the delay ring");
        }
    expect(band_chain_plan(10000, 10000, 512, false).unit_delay && band_chain_plan(10000, 10000, 512, false).d == 17, "BASELINE configuration 5: unit delay");
    // where the chain is not built, by reason (then the strips run)
    expect(std::string(fallback_reason(band_chain_plan(1, 81, 100000, false))) == "fill", "more than two rounds of reference per event");
    expect(std::string(fallback_reason(band_chain_plan(2, 3853, 64, false))) == "code_cols", "a reference ring beyond 2048 columns");
    expect(std::string(fallback_reason(band_chain_plan(1, 1, 100000, false))) == "ring", "a delay ring beyond 64 slots");
    // LDS: linear gaps never reach 40 KiB (10240 + 4096 + 64 x 64 x 4 = 30720 at the largest rings); the second ring of the
    // affine kernels does, at a ring depth of 64 -- which is where affine flips `usable`
    expect(BandLds<16>::total(2048, 64) == 30720 && BandLds<16>::total(128, 64, true) > 40 * 1024, "the LDS limit");
    const BandPlan lin = band_chain_plan(1, 1, 2000, false), aff = band_chain_plan(1, 1, 2000, true);
    expect(lin.usable && lin.ring_depth == 64 && !aff.usable && std::string(fallback_reason(aff)) == "lds", "affine gaps flip usable through LDS");
}

int print_plans() {
    int R, F, band;
    while (scanf("%d %d %d", &R, &F, &band) == 3) {
        const BandPlan p = band_chain_plan(R, F, band, false);
        printf("%d %d %d %d %d %d %d\n", R, F, band, p.nb, p.pad_rows, p.d, p.unit_delay ? 1 : 0);
        for (int b = 0; b < p.nb; ++b) printf("%d %d %d ", p.blocks[(size_t)b].start, p.blocks[(size_t)b].lo, p.blocks[(size_t)b].span);
        printf("\n");
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "--plans")) return print_plans();
    check_routes();
    check_edges();
    check_instances();
    check_sizes();
    check_chain();
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("long plan ok\n");
    return 0;
}
