// sym_affine_side_tile_rules_check.cpp -- the rule that hands out the 8 x 19 side tile of the tilted int16 symmetric affine
// Smith-Waterman sweep (versalignlib_amd/csrc/cell_rules.h: sym_affine_side_tile_refusal), on the CPU: plain g++, no HIP.
//   1. the traits: the tilted frame is built for K <= kTiltMaxK and for 8 x 19 only, and sym_affine_tilt_ok reads them;
//   2. every condition of the rule at its edge, each with a text of its own: the algorithm, the gap form, the read length
//      (128 / 129, 152 / 153), the three debug words, the bytes of the row tables (255 / 256, 0 / -1), the tilted window,
//      the LDS budget (two 4-wave blocks per CU with a margin), the latency plan;
//   3. a forced tile: no lower bound on the read and no latency plan, everything else as it stands;
//   4. the older rules answer as before whatever the new switch says;
//   5. the numbers the GPU edge tests run at, as literals: the last reference the LDS budget takes (558, 19,456 B per wave), the
//      stream stride's five values and where each begins, the last match score inside the tilted window per shape and scoring.
#include <cstdio>
#include <cstring>
#include <string>

#include "cell_rules.h"

using namespace valign;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            if (failures < 20) printf("FAILED line %d: %s\n", __LINE__, #cond); \
        }                                                                  \
    } while (0)

static Scoring aff(int m, int mm, int open, int ext) { return Scoring{m, mm, -3, -3, true, open, ext, open, ext}; }

static RuleInputs inputs(const Scoring &sc, int R, int F) {
    RuleInputs in;
    in.sc = sc;
    in.R = R;
    in.F = F;
    return in;
}

constexpr int kLds500 = 16480;       // bytes per wave of the side plan at 150 x 500 (cell_constants.h: side_tile_wave_lds)

static std::string why(const RuleInputs &in, int alg, int gaps, bool latency = false, bool forced = false) {
    return sym_affine_side_tile_refusal(in, alg, gaps, in.R, in.F, latency, forced);
}
static bool has(const std::string &text, const char *piece) { return text.find(piece) != std::string::npos; }

int main() {
    const Scoring bench = aff(2, -1, -5, -1);

    // 1. the traits
    CHECK(tilt_tables_only(8, 19) && !tilt_tables_only(16, 19) && !tilt_tables_only(8, 20) && !tilt_tables_only(8, 12));
    CHECK(tilt_frame_built(8, 19) && tilt_frame_built(16, 10) && tilt_frame_built(64, 12) && !tilt_frame_built(64, 16) && !tilt_frame_built(16, 19) &&
          !tilt_frame_built(8, 20));
    CHECK(kTiltMaxK == 12 && kSideTileRows == 152 && kSideTileMinRead == 129);
    {
        const RuleInputs in = inputs(bench, 150, 500);
        CHECK(sym_affine_tilt_ok(in, 150, 500, 152, 19) && sym_affine_tilt_ok(in, 150, 500, 160, 10));
        CHECK(!sym_affine_tilt_ok(in, 150, 500, 304, 19) && !sym_affine_tilt_ok(in, 150, 500, 160, 20) && !sym_affine_tilt_ok(in, 150, 500, 1024, 16));
        CHECK(sym_affine_tilt_top_index(150, 500, 152, 19) == 652 && sym_affine_tilt_top_index(1, 500, 152, 19) == 652 - 7);
    }

    // 2. the conditions, one by one
    {
        RuleInputs in = inputs(bench, 150, 500);
        CHECK(why(in, kAlgSW, kGapAffineSym).empty());
        CHECK(has(why(in, kAlgNW, kGapAffineSym), "Smith-Waterman"));
        for (int gaps : {kGapLinear, kGapSym, kGapAffine, kGapAffineSymF16, kGapAffineF16, kGapSymF16}) CHECK(has(why(in, kAlgSW, gaps), "int16 cells with symmetric affine gaps"));
        // the read length
        for (int R : {129, 133, 150, 151, 152}) CHECK(why(inputs(bench, R, 500), kAlgSW, kGapAffineSym).empty());
        CHECK(has(why(inputs(bench, 128, 500), kAlgSW, kGapAffineSym), "at most 128") && has(why(inputs(bench, 1, 500), kAlgSW, kGapAffineSym), "at most 128"));
        CHECK(has(why(inputs(bench, 153, 500), kAlgSW, kGapAffineSym), "at most 152"));
        // the debug words
        in.no_side_tile = true;
        CHECK(has(why(in, kAlgSW, kGapAffineSym), "no_side_tile"));
        in.no_side_tile = false;
        in.no_tilt = true;
        CHECK(has(why(in, kAlgSW, kGapAffineSym), "no_tilt"));
        in.no_tilt = false;
        in.no_row_tables = true;
        CHECK(has(why(in, kAlgSW, kGapAffineSym), "no_row_tables"));
        in.no_row_tables = false;
        in.no_max3 = true;
        CHECK(has(why(in, kAlgSW, kGapAffineSym), "sym_affine_row_tables_ok"));
        in.no_max3 = false;
        // the latency plan
        CHECK(has(why(in, kAlgSW, kGapAffineSym, true), "latency"));
        // the bytes: the largest 255 / 256, the smallest 0 / -1 (short references: inside the tilted window whatever the match score)
        CHECK(why(inputs(aff(249, -1, -5, -1), 150, 39), kAlgSW, kGapAffineSym).empty());
        CHECK(has(why(inputs(aff(250, -1, -5, -1), 150, 39), kAlgSW, kGapAffineSym), "no byte"));
        CHECK(why(inputs(aff(2, -2, -5, -1), 150, 500), kAlgSW, kGapAffineSym).empty());
        CHECK(has(why(inputs(aff(2, -3, -5, -1), 150, 500), kAlgSW, kGapAffineSym), "no byte"));
        CHECK(has(why(inputs(aff(2, -1, -2, -3), 150, 500), kAlgSW, kGapAffineSym), "sym_affine_row_tables_ok"));      // o - x < 0
        // the tilted window on 152 rows of 19: the last match score inside it and the first outside
        {
            int edge = 0;
            for (int m = 1; m < 400; ++m)
                if (sym_affine_tilt_ok(inputs(aff(m, -1, -5, -1), 150, 500), 150, 500, 152, 19)) edge = m;
            const long long B = sym_affine_tilt_bias(aff(edge, -1, -5, -1));
            CHECK(edge > 2 && edge < 249);
            CHECK(B + 652 + 150ll * edge + 1 <= kMax3WindowHigh && B + 652 + 150ll * (edge + 1) + 1 > kMax3WindowHigh);
            CHECK(why(inputs(aff(edge, -1, -5, -1), 150, 500), kAlgSW, kGapAffineSym).empty());
            CHECK(has(why(inputs(aff(edge + 1, -1, -5, -1), 150, 500), kAlgSW, kGapAffineSym), "window"));
        }
        // the LDS budget: each 4-wave block rounded up to 2 KB, two of them inside 152 KB
        CHECK(side_tile_lds_ok(kLds500) && side_tile_lds_ok(19456) && !side_tile_lds_ok(19457) && !side_tile_lds_ok(0) && !side_tile_lds_ok(26720));
        CHECK(2 * 4 * 19456 == kSideTileLdsBudget && kSideTileLdsBudget < 160 * 1024);
        // ... which the rule sizes itself: 16 raw references + 8 streams of 16 bits per column, the stride 8 (mod 64) dwords
        CHECK(side_tile_wave_lds(150, 500) == kLds500 && side_tile_refs_area(500) == 8032 && side_tile_stream_stride(500) == 1056);
        CHECK(side_tile_stream_stride(1) % 256 == 32 && side_tile_stream_stride(39) % 256 == 32 && side_tile_stream_stride(500) % 256 == 32);
        CHECK(side_tile_wave_lds(150, 1) == 48 + 2432);                                  // (a short reference: the staged reads are the larger)
        {
            int last = 0;                   // the longest reference whose two blocks fit
            for (int F = 1; F < 2000; ++F)
                if (side_tile_lds_ok(side_tile_wave_lds(150, F))) last = F;
            CHECK(last > 500 && last < 700 && side_tile_wave_lds(150, last) <= 19456 && side_tile_wave_lds(150, last + 1) > 19456);
            CHECK(why(inputs(bench, 150, last), kAlgSW, kGapAffineSym).empty());
            CHECK(has(why(inputs(bench, 150, last + 1), kAlgSW, kGapAffineSym), "two 4-wave blocks"));
            // a length-sorted launch: the LDS of ITS shape, the windows of the engine's
            CHECK(std::string(sym_affine_side_tile_refusal(inputs(bench, 150, last + 1), kAlgSW, kGapAffineSym, 150, 64, false, false)).empty());
        }
    }

    // 3. forced
    {
        CHECK(why(inputs(bench, 1, 64), kAlgSW, kGapAffineSym, false, true).empty());
        CHECK(why(inputs(bench, 128, 64), kAlgSW, kGapAffineSym, true, true).empty());
        CHECK(why(inputs(bench, 152, 64), kAlgSW, kGapAffineSym, true, true).empty());
        CHECK(has(why(inputs(bench, 153, 64), kAlgSW, kGapAffineSym, false, true), "at most 152"));
        CHECK(has(why(inputs(aff(2, -3, -5, -1), 150, 64), kAlgSW, kGapAffineSym, false, true), "no byte"));
        CHECK(has(why(inputs(bench, 150, 64), kAlgNW, kGapAffineSym, false, true), "Smith-Waterman"));
        CHECK(has(why(inputs(bench, 150, 64), kAlgSW, kGapAffineSymF16, false, true), "int16 cells"));
        CHECK(has(why(inputs(bench, 150, 700), kAlgSW, kGapAffineSym, false, true), "two 4-wave blocks"));
        RuleInputs in = inputs(bench, 150, 64);
        in.no_side_tile = true;
        CHECK(has(why(in, kAlgSW, kGapAffineSym, false, true), "no_side_tile"));
    }

    // 4. the older rules do not read the new switch
    {
        RuleInputs in = inputs(bench, 150, 500);
        const bool tilt = sym_affine_tilt_ok(in, 150, 500, 160, 10), tables = sym_affine_row_tables_ok(in, 150, 500, 160, 10, 1000, 1000);
        const int form = score_gap_form(in, kAlgSW, 150, 500, 160);
        in.no_side_tile = true;
        CHECK(tilt && tables && sym_affine_tilt_ok(in, 150, 500, 160, 10) && sym_affine_row_tables_ok(in, 150, 500, 160, 10, 1000, 1000));
        CHECK(score_gap_form(in, kAlgSW, 150, 500, 160) == form);
    }

    // 5. the literals tests/test_gpu_sym_affine_side_tile_edges.py runs the kernel at: they are THIS arithmetic's, so a header that
    //    moves an edge fails here and not by silently moving what the GPU tests cover
    {
        // the LDS budget's edge: F = 558 fills two 4-wave blocks to the byte, whatever the read (the streams are the larger area)
        for (int R : {129, 150, 152}) {
            int last = 0;
            for (int F = 1; F < 2000; ++F)
                if (side_tile_lds_ok(side_tile_wave_lds(R, F))) last = F;
            CHECK(last == 558);
            CHECK(side_tile_wave_lds(R, 558) == 19456 && side_tile_wave_lds(R, 559) == 19472);
            CHECK(2 * kSideTileBlockWaves * side_tile_wave_lds(R, 558) == kSideTileLdsBudget);
            CHECK(why(inputs(bench, R, 558), kAlgSW, kGapAffineSym, false, true).empty());
            CHECK(has(why(inputs(bench, R, 559), kAlgSW, kGapAffineSym, false, true), "too long for its LDS budget"));
        }
        // the stream stride's steps: five values up to the budget's edge, and the reference length at which each begins
        const int strides[5][2] = {{1, 288}, {121, 544}, {249, 800}, {377, 1056}, {505, 1312}};
        int step = 0, prev = 0;
        for (int F = 1; F <= 559; ++F) {
            const int s = side_tile_stream_stride(F);
            if (s != prev) {
                CHECK(step < 5 && strides[step][0] == F && strides[step][1] == s);
                ++step;
                prev = s;
            }
            CHECK(s % 256 == 32 && s >= 2 * (F + 2 * kSideTilePad));         // 8 (mod 64) dwords, and room for every column and both pads
        }
        CHECK(step == 5);
        // the tilted window's edge on 152 rows of 19: the last match score the forced tile runs, the first it refuses -- by the
        // window, not by the bytes, which pass at both
        const struct {
            int R, F, mismatch, open, ext, edge;
        } edges[] = {{152, 152, -1, -5, -1, 200}, {152, 558, -1, -5, -1, 197},  {150, 500, -1, -5, -1, 200},
                     {152, 558, -20, -24, -20, 108}, {133, 558, -20, -24, -20, 124}};
        for (const auto &e : edges) {
            const Scoring at = aff(e.edge, e.mismatch, e.open, e.ext), past = aff(e.edge + 1, e.mismatch, e.open, e.ext);
            CHECK(why(inputs(at, e.R, e.F), kAlgSW, kGapAffineSym, false, true).empty());
            CHECK(has(why(inputs(past, e.R, e.F), kAlgSW, kGapAffineSym, false, true), "sym_affine_row_tables_ok"));
            CHECK(sym_affine_tilt_ok(inputs(at, e.R, e.F), e.R, e.F, kSideTileRows, kSideTileK) &&
                  !sym_affine_tilt_ok(inputs(past, e.R, e.F), e.R, e.F, kSideTileRows, kSideTileK));
            CHECK(sym_affine_max3_ok(inputs(past, e.R, e.F), e.R, e.F));                 // (the plain biased form's window is not what refuses)
            for (const Scoring &sc : {at, past}) CHECK(sym_affine_row_table_low(sc) >= 0 && sym_affine_row_table_high(sc) <= 255 && sc.ext_ref - sc.open_ref >= 0);
            const long long lead = (kSideTileRows - e.R) / kSideTileK, top = kSideTileRows + e.F - lead;
            CHECK(sym_affine_tilt_top_index(e.R, e.F, kSideTileRows, kSideTileK) == top);
            const long long B = sym_affine_tilt_bias(at), room = kMax3WindowHigh - 1 - B - (long long)-e.ext * top;
            CHECK(B == sym_affine_tilt_bias(past) && room / std::min(e.R, e.F) == e.edge);
        }
        CHECK(sym_affine_tilt_top_index(133, 558, kSideTileRows, kSideTileK) == 709 && sym_affine_tilt_top_index(152, 558, kSideTileRows, kSideTileK) == 710);
    }

    if (failures) {
        printf("%d check(s) FAILED\n", failures);
        return 1;
    }
    printf("sym affine side tile rules ok\n");
    return 0;
}
