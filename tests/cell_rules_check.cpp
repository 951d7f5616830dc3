// cell_rules_check.cpp -- CPU check of versalignlib_amd/csrc/cell_rules.h: the closed-form bounds that pick cell format, fill
// kernel and path of every call.  It includes that header alone -- that this compiles with plain g++, without HIP, is the
// first assertion -- and checks what needs no tolerance (tests/test_cell_rules.py builds and runs it; tools/sanitize.sh
// runs it under UBSan):
//   1. score_gap_form is a half-float form exactly where the half_float_* predicate of the mode holds and no_f16 is off;
//   2. every family tests/test_gpu_range_edges.py walks on the GPU, restated in FAMILIES below (same shape, scoring family
//      and range): narrow at lo, not at hi, exactly one change in between (the GPU test's bisection assumes it), and the
//      change where that test pins it;
//   3. the route of an alignment call: refusals before every route, Fused only where every fused geometry fills with a plain
//      tag kernel, strip-sized chunks exactly where align_host's former by_strips expression held.
#include "cell_rules.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>

using namespace valign;

namespace {

int failures = 0;
void expect(bool ok, const std::string &what) {
    if (!ok && ++failures <= 20) fprintf(stderr, "FAIL: %s\n", what.c_str());
}

uint64_t rng_state = 1;
uint64_t rnd() {        // splitmix64
    uint64_t x = (rng_state += 0x9E3779B97F4A7C15ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
int pick(std::initializer_list<int> v) { return v.begin()[rnd() % v.size()]; }

// as the Python wrapper builds it: without affine scores the open / extend fields repeat the gap scores
Scoring lin(int m, int mm, int gr, int gf) { return Scoring{m, mm, gr, gf, false, gr, gr, gf, gf}; }
Scoring aff(int m, int mm, int g, int orr, int er, int of, int ef) { return Scoring{m, mm, g, g, true, orr, er, of, ef}; }

std::string describe(const RuleInputs &in, int alg) {
    char buf[256];
    snprintf(buf, sizeof buf, "alg %d %dx%d m %d mm %d g %d/%d affine %d o/e %d/%d %d/%d sse %d", alg, in.R, in.F, in.sc.match, in.sc.mismatch,
             in.sc.gap_read, in.sc.gap_ref, in.sc.affine, in.sc.open_read, in.sc.ext_read, in.sc.open_ref, in.sc.ext_ref, in.sse_policy);
    return buf;
}

// ---- 1. the gap form of a score launch ----
void check_gap_forms() {
    const int shapes[][3] = {{150, 500, 160}, {150, 500, 256}, {64, 128, 64}, {50, 100, 64}, {1000, 2000, 1024}, {9, 5, 512}, {300, 40, 320}};
    long long f16_forms = 0, cases = 0;
    for (const auto &shape : shapes)
        for (int m : {1, 2, 4, 5, 6, 7, 11, 12, 13, 14, 30, 700})
            for (int mm : {-1, -11, -210, -211, -361, -362, -512, -513, -1100})
                for (int g : {0, -1, -3, -4, -5, -20, -600})
                    for (int kind = 0; kind < 4; ++kind)          // linear one gap score / two; affine symmetric / not
                        for (int alg : {kAlgSW, kAlgNW})
                            for (int sw = 0; sw < 4; ++sw) {
                                RuleInputs in;
                                in.sc = kind == 0 ? lin(m, mm, g, g) : kind == 1 ? lin(m, mm, g, g - 1) : kind == 2 ? aff(m, mm, g, g - 17, g, g - 17, g) : aff(m, mm, g, g - 17, g, g - 18, g - 1);
                                in.R = shape[0];
                                in.F = shape[1];
                                in.no_f16 = sw & 1;
                                in.no_sym = sw & 2;
                                const int form = score_gap_form(in, alg, in.R, in.F, shape[2]);
                                const bool sym = kind == 0 && !in.no_sym;
                                // the predicate of the mode: affine gaps and the NW variant's tilted frame on +-2048 integers; linear SW
                                // (one gap score only: the clamp needs it) on the unit scale
                                const bool exact = (in.sc.affine || alg == kAlgNW) ? half_float_exact(in.sc, alg, in.R, in.F, shape[2])
                                                                                  : (sym && half_float_unit_exact(in.sc, in.R, in.F));
                                expect(gap_form_f16(form) == (exact && !in.no_f16), "gap form " + std::to_string(form) + ": " + describe(in, alg));
                                expect((form == kGapAffine || form == kGapAffineSym || form == kGapAffineSymF16 || form == kGapAffineF16) == in.sc.affine, "affine form: " + describe(in, alg));
                                f16_forms += gap_form_f16(form);
                                ++cases;
                            }
    expect(f16_forms > cases / 50 && f16_forms < cases / 2, "the grid reaches both sides of the half-float rules");
}

// ---- 2. the walked families of tests/test_gpu_range_edges.py ----
struct Family {
    const char *id;
    bool score;                     // a score call (else an alignment call)
    int alg, R, F, lo, hi;
    Scoring (*sc)(int v);
    const char *narrow;             // what counts as the narrow form, names between commas
    int last_narrow;                // EDGES of the GPU test: narrow up to here, the other form from the next value on
    int G, K;                       // alignments: the geometry the call runs on (150 x 500: 16 x 10; a forced one where the row forces it)
    int rows;                       // scores: padded rows of the plan the call sweeps on (small calls: the latency plan's 256; large: 160)
    bool sse, small_call, long_mode;
    int walk;                       // 0: the scoring; 1: read_length; 2: ref_length
};
#define NOT_INT32 ",f16,int16,"
#define NOT_WIDE ",fused_tag,tag_prof_key,tag_key,tag,sse_tag_key,sse_tag,sse,affine_tag_sym,affine_tag,affine_sym,affine,linear_sym,linear,strip,"
const Family FAMILIES[] = {
    {"half_float_exact-sw", true, kAlgSW, 150, 500, 1, 30, [](int v) { return aff(v, -11, -20, -20, -3, -20, -3); }, ",f16,", 13, 0, 0, 256, false, false, false, 0},
    {"half_float_exact_small_call-nw", true, kAlgNW, 150, 500, 1, 30, [](int v) { return aff(v, -11, -20, -20, -3, -20, -3); }, ",f16,", 11, 0, 0, 256, false, false, false, 0},
    {"half_float_exact_large_call-nw", true, kAlgNW, 150, 500, 1, 30, [](int v) { return aff(v, -11, -20, -20, -3, -20, -3); }, ",f16,", 13, 0, 0, 160, false, false, false, 0},
    {"half_float_exact_linear-nw", true, kAlgNW, 150, 500, 1, 20, [](int v) { return lin(2, -1, -v, -v); }, ",f16,", 4, 0, 0, 256, false, false, false, 0},
    {"half_float_exact_mismatch-nw", true, kAlgNW, 150, 500, 50, 700, [](int v) { return lin(2, -v, -1, -1); }, ",f16,", 210, 0, 0, 256, false, false, false, 0},
    {"half_float_exact_slack-nw", true, kAlgNW, 50, 100, 400, 600, [](int v) { return lin(1, -v, 0, 0); }, ",f16,", 512, 0, 0, 64, false, false, false, 0},
    {"half_float_unit_exact-sw", true, kAlgSW, 150, 500, 1, 12, [](int v) { return lin(v, -1, -3, -3); }, ",f16,", 6, 0, 0, 256, false, false, false, 0},
    {"half_float_unit_exact_slack-sw", true, kAlgSW, 150, 500, 100, 600, [](int v) { return lin(2, -v, -3, -3); }, ",f16,", 361, 0, 0, 256, false, false, false, 0},
    {"half_float_unit_exact_long-sw", true, kAlgSW, 150, 8000, 1, 12, [](int v) { return lin(v, -1, -3, -3); }, ",f16,", 6, 0, 0, 160, false, false, true, 0},
    {"int16_range_score-sw", true, kAlgSW, 150, 500, 150, 300, [](int v) { return lin(v, -1, -3, -3); }, NOT_INT32, 213, 0, 0, 256, false, false, false, 0},
    {"int16_range_read_length-sw", true, kAlgSW, 150, 500, 140, 180, [](int) { return lin(200, -1, -3, -3); }, NOT_INT32, 159, 0, 0, 256, false, false, false, 1},
    {"int16_range_score-nw", true, kAlgNW, 150, 500, 150, 300, [](int v) { return lin(2, -v, -1, -1); }, NOT_INT32, 210, 0, 0, 256, false, false, false, 0},
    {"int16_range_score_affine_nw_lo-nw", true, kAlgNW, 150, 500, 60, 200, [](int v) { return aff(2, -v, -5, -5, -1, -5, -1); }, NOT_INT32, 98, 0, 0, 256, false, false, false, 0},
    {"int16_range_align-sw", false, kAlgSW, 150, 500, 150, 300, [](int v) { return lin(v, -1, -3, -3); }, NOT_WIDE, 213, 16, 10, 0, false, false, false, 0},
    {"int16_range_align_abi-sw", false, kAlgSW, 150, 500, 150, 300, [](int v) { return lin(v, -1, -3, -3); }, NOT_WIDE, 213, 16, 10, 0, false, true, false, 0},
    {"int16_range_align-nw", false, kAlgNW, 150, 500, 150, 300, [](int v) { return lin(2, -v, -1, -1); }, NOT_WIDE, 210, 16, 10, 0, false, false, false, 0},
    {"int16_range_align_abi-nw", false, kAlgNW, 150, 500, 150, 300, [](int v) { return lin(2, -v, -1, -1); }, NOT_WIDE, 210, 16, 10, 0, false, true, false, 0},
    {"int16_range_align_affine_nw_lo-nw", false, kAlgNW, 150, 500, 60, 200, [](int v) { return aff(2, -1, -v, -v, -v, -v, -v); }, NOT_WIDE, 98, 16, 10, 0, false, false, false, 0},
    {"border_bad-nw", false, kAlgNW, 400, 50, 40, 120, [](int v) { return lin(2, -1, -1, -v); }, NOT_WIDE, 79, 64, 8, 0, false, false, false, 0},
    {"prof_key-sw", false, kAlgSW, 150, 500, 1, 20, [](int v) { return lin(v, -1, -3, -3); }, ",tag_prof_key,", 3, 16, 10, 0, false, false, false, 0},
    {"prof_key_mismatch-sw", false, kAlgSW, 150, 500, 200, 300, [](int v) { return lin(1, -v, -3, -3); }, ",tag_prof_key,", 249, 16, 10, 0, false, false, false, 0},
    {"prof_key_gap-sw", false, kAlgSW, 150, 500, 450, 550, [](int v) { return lin(1, -1, -v, -v); }, ",tag_prof_key,", 499, 16, 10, 0, false, false, false, 0},
    {"lane_key-sw", false, kAlgSW, 150, 500, 1, 40, [](int v) { return lin(v, -1, -3, -3); }, ",tag_prof_key,tag_key,", 13, 16, 10, 0, false, false, false, 0},
    {"lane_key_5bit-sw", false, kAlgSW, 150, 500, 1, 40, [](int v) { return lin(v, -1, -3, -3); }, ",tag_key,", 6, 64, 32, 0, false, false, false, 0},
    {"tagged-sw", false, kAlgSW, 150, 500, 20, 100, [](int v) { return lin(v, -1, -3, -3); }, ",tag_prof_key,tag_key,tag,", 53, 16, 10, 0, false, false, false, 0},
    {"tagged-nw", false, kAlgNW, 150, 500, 20, 100, [](int v) { return lin(v, -1, -1, -1); }, ",tag,", 48, 16, 10, 0, false, false, false, 0},
    {"tagged_mismatch-sw", false, kAlgSW, 150, 500, 1900, 2100, [](int v) { return lin(1, -v, -3, -3); }, ",tag_key,", 1999, 16, 10, 0, false, false, false, 0},
    {"tagged_lo_gap-sw", false, kAlgSW, 150, 500, 7900, 8100, [](int v) { return lin(1, -1, -v, -v); }, ",tag_key,", 7999, 16, 10, 0, false, false, false, 0},
    {"tagged_lo-nw", false, kAlgNW, 150, 500, 2, 40, [](int v) { return lin(2, -v, -1, -1); }, ",tag,", 12, 16, 10, 0, false, false, false, 0},
    {"sse_lane_key-sw", false, kAlgSW, 150, 500, 1, 40, [](int v) { return lin(v, -1, -3, -3); }, ",sse_tag_key,", 13, 16, 10, 0, true, false, false, 0},
    {"sse_tagged-sw", false, kAlgSW, 150, 500, 20, 100, [](int v) { return lin(v, -1, -3, -3); }, ",sse_tag_key,sse_tag,", 53, 16, 10, 0, true, false, false, 0},
    {"sse_tagged-nw", false, kAlgNW, 150, 500, 2, 40, [](int v) { return lin(2, -v, -1, -1); }, ",sse_tag,", 12, 16, 10, 0, true, false, false, 0},
    {"affine_tagged-sw", false, kAlgSW, 150, 500, 1, 40, [](int v) { return aff(v, -1, -5, -5, -1, -5, -1); }, ",affine_tag_sym,", 13, 16, 10, 0, false, false, false, 0},
    {"affine_tagged_asym-sw", false, kAlgSW, 150, 500, 1, 40, [](int v) { return aff(v, -1, -5, -5, -1, -6, -2); }, ",affine_tag,", 13, 16, 10, 0, false, false, false, 0},
    {"affine_tagged_lo-nw", false, kAlgNW, 150, 500, 100, 900, [](int v) { return aff(2, -1, -v, -v, -1, -v, -1); }, ",affine_tag_sym,", 569, 16, 10, 0, false, false, false, 0},
    {"affine_tagged_hi-nw", false, kAlgNW, 150, 500, 2, 40, [](int v) { return aff(v, -1, -5, -5, -1, -5, -1); }, ",affine_tag_sym,", 22, 16, 10, 0, false, false, false, 0},
    {"affine_tagged_hi_ref_length-nw", false, kAlgNW, 150, 500, 500, 600, [](int) { return aff(22, -1, -5, -5, -1, -5, -1); }, ",affine_tag_sym,", 536, 16, 10, 0, false, false, false, 2},
    {"affine_tagged_tilt-nw", false, kAlgNW, 9, 5, 2, 20, [](int v) { Scoring s = aff(1, -1, -1, -1, -1, -v, -v); s.gap_ref = -v; return s; }, ",affine_tag,", 6, 64, 8, 0, false, false, false, 0},
    {"affine_tagged_5bit-sw", false, kAlgSW, 150, 500, 1, 40, [](int v) { return aff(v, -1, -5, -5, -1, -5, -1); }, ",affine_tag_sym,", 6, 64, 32, 0, false, false, false, 0},
    {"affine_tagged_mismatch-sw", false, kAlgSW, 150, 500, 900, 1100, [](int v) { return aff(2, -v, -5, -5, -1, -5, -1); }, ",affine_tag_sym,", 999, 16, 10, 0, false, false, false, 0},
    {"fused-sw", false, kAlgSW, 64, 128, 60, 200, [](int v) { return lin(v, -1, -3, -3); }, ",fused_tag,", 124, 8, 8, 0, false, true, false, 0},
    {"fused-nw", false, kAlgNW, 64, 128, 60, 200, [](int v) { return lin(v, -1, -1, -1); }, ",fused_tag,", 118, 8, 8, 0, false, true, false, 0},
};

constexpr int kFusedRows = 256;         // 64 x 4, the tallest fused geometry

// what a call of the family reports it ran at walked value v (ran_score_cells / ran_align_fill), from the rules alone
std::string ran(const Family &f, int v) {
    RuleInputs in;
    in.sc = f.sc(v);
    in.R = f.walk == 1 ? v : f.R;
    in.F = f.walk == 2 ? v : f.F;
    in.sse_policy = f.sse;
    if (f.score) {
        if (!int16_range_ok(in, f.alg, true, f.long_mode, kFusedRows)) return "int32";      // (tilt: the latency plan's 256 rows)
        if (f.long_mode) return (f.alg == kAlgSW && !in.sc.affine && in.sc.gap_read == in.sc.gap_ref && half_float_unit_exact(in.sc, in.R, in.F)) ? "f16" : "int16";
        return gap_form_f16(score_gap_form(in, f.alg, in.R, in.F, f.rows)) ? "f16" : "int16";
    }
    const RouteFacts facts{false, false, false, false, f.small_call, kFusedRows};      // (the rows through the ABI force no geometry)
    return ran_fill_name(align_route(in, f.alg, facts), fill_choice(in, f.alg, f.G, f.K).kernel);
}

void check_families() {
    for (const Family &f : FAMILIES) {
        auto narrow = [&](int v) { return strstr(f.narrow, ("," + ran(f, v) + ",").c_str()) != nullptr; };
        expect(narrow(f.lo), std::string(f.id) + ": not narrow at lo (" + ran(f, f.lo) + ")");
        expect(!narrow(f.hi), std::string(f.id) + ": still narrow at hi (" + ran(f, f.hi) + ")");
        int changes = 0, last = f.lo;
        for (int v = f.lo; v < f.hi; ++v) {
            if (narrow(v) != narrow(v + 1)) ++changes;
            if (narrow(v)) last = v;
        }
        expect(changes == 1, std::string(f.id) + ": " + std::to_string(changes) + " changes inside the walk");
        expect(last == f.last_narrow, std::string(f.id) + ": narrow up to " + std::to_string(last) + ", the GPU test pins " + std::to_string(f.last_narrow));
    }
}

// ---- 3. the route of an alignment call ----
bool route_throws(const RuleInputs &in, int alg, const RouteFacts &f, AlignRoute &route, std::string &what) {
    try {
        route = align_route(in, alg, f);
        return false;
    } catch (const std::runtime_error &e) {
        what = e.what();
        return true;
    }
}

void check_routes() {
    const int fused_geometries[][2] = {{8, 4}, {16, 4}, {32, 2}, {16, 8}, {32, 4}, {16, 10}, {32, 8}, {64, 4}};
    long long seen[6] = {}, refused = 0;
    for (int it = 0; it < 400000; ++it) {
        RuleInputs in;
        const int m = pick({1, 2, 5, 60, 124, 125, 200, 300, 5000, 32760, 32761}), mm = -pick({0, 1, 4, 200, 2000, 32761});
        const int g = -pick({0, 1, 3, 79, 80, 500, 8000, 32761}), g2 = rnd() % 2 ? g : -pick({1, 80, 9000});
        in.sc = rnd() % 2 ? lin(m, mm, g, g2) : aff(m, mm, g, g - pick({0, 5, 700}), g, g2 - pick({0, 5, 700}), g2);
        in.R = pick({1, 9, 64, 150, 400, 1024, 1025, 10000});
        in.F = pick({5, 50, 128, 500, 8092, 10000});
        in.sse_policy = rnd() % 4 == 0;
        in.no_tag = rnd() % 8 == 0;
        const int alg = rnd() % 2;
        RouteFacts f;
        f.banded = rnd() % 4 == 0;
        f.wide_align = rnd() % 8 == 0;
        f.read_strips = in.R > 1024 || rnd() % 4 == 0;
        f.fused_off = rnd() % 4 == 0;
        f.small_call = rnd() % 2;
        f.fused_rows = kFusedRows;
        AlignRoute route = AlignRoute::Register;
        std::string what;
        const bool threw = route_throws(in, alg, f, route, what);
        // the refusals, restated: band_alignments with NW or with traceback_policy = 1; cells beyond int16 whose scores near 2^28
        const bool wide = border_bad(in, alg) || !int16_range_ok(in, alg, false, false, 0) || f.wide_align;
        const bool band_refused = f.banded && (alg != kAlgSW || in.sse_policy);
        const bool refusal = band_refused || (wide && int32_refused(in));
        if (refusal) {
            expect(threw, "a refusal yields to no route: " + describe(in, alg));
            expect(band_refused ? what.find("band_alignments") == 0 : what.find("int32 range") != std::string::npos, "refusal text '" + what + "': " + describe(in, alg));
            // ... whatever the other facts say
            RouteFacts other = f;
            other.read_strips = !f.read_strips;
            other.small_call = !f.small_call;
            other.fused_off = !f.fused_off;
            expect(route_throws(in, alg, other, route, what), "a refusal does not depend on the path: " + describe(in, alg));
            ++refused;
            continue;
        }
        // by_strips as align_host had it: the long-read plan or an unforced read beyond 1 024 rows (read_strips), or the band
        const bool old_by_strips = f.read_strips || f.banded;
        if (threw) {        // what is left: SSE tie-breaks with affine gaps, met only on the register / fused side of the cascade
            expect(in.sse_policy && in.sc.affine && !wide && !old_by_strips && what.find("traceback_policy = 1") == 0, "unexpected refusal '" + what + "': " + describe(in, alg));
            ++refused;
            continue;
        }
        ++seen[(int)route];
        expect(strip_chunks(route, f) == old_by_strips, "strip chunks: " + describe(in, alg));
        const bool wide_route = route == AlignRoute::StripWide || route == AlignRoute::StripWideBand;
        const bool band_route = route == AlignRoute::StripBand || route == AlignRoute::StripWideBand;
        expect(wide_route == wide && band_route == f.banded, "int32 cells / band of the route: " + describe(in, alg));
        expect((route == AlignRoute::Strip) == (!wide && !f.banded && f.read_strips), "plain strips: " + describe(in, alg));
        if (route == AlignRoute::Fused) {
            expect(f.small_call && !f.fused_off && !in.sc.affine && !in.sse_policy, "Fused for a call that may not fuse: " + describe(in, alg));
            for (const auto &geo : fused_geometries) {
                const FillChoice c = fill_choice(in, alg, geo[0], geo[1]);
                expect(c.tagged && !c.affine_tagged && (c.kernel == kFillTag || c.kernel == kFillTagKey || c.kernel == kFillTagProfKey),
                       "Fused where " + std::to_string(geo[0]) + " x " + std::to_string(geo[1]) + " fills with no plain tag kernel: " + describe(in, alg));
            }
        }
    }
    for (int r = 0; r < 6; ++r) expect(seen[r] > 100, "route " + std::to_string(r) + " reached");
    expect(refused > 1000, "refusals reached");
}

}  // namespace

int main() {
    check_gap_forms();
    check_families();
    check_routes();
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("cell rules ok\n");
    return 0;
}
