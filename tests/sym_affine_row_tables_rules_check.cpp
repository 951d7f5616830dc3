// sym_affine_row_tables_rules_check.cpp -- the rule behind the ROW TABLES of the tilted int16 symmetric affine Smith-Waterman sweep
// (versalignlib_amd/csrc/cell_rules.h: sym_affine_row_tables_ok), on the CPU: plain g++, no HIP.
//   1. the table bytes: with x = -extend and o = -open, match' = match + 2x, mismatch' = mismatch + 2x, zero' = 2x and, on a lane's
//      row 0, each plus o - x.  The rule flips exactly between a largest byte of 255 and 256, and between mismatch' = 0 and -1
//      (match' likewise); o - x < 0 is refused.
//   2. it is false wherever sym_affine_tilt_ok is, under no_row_tables, and where the tables' LDS would exceed the plan's.
//   3. the window: for every scoring the rule accepts, the smallest diagonal candidate a column scoring 0 can produce -- B + x
//      (rows 1 .. K-1: floor - 2x at u >= 3) and B - (o - x) (row 0: floor - o - x at u >= 2) -- is at or above 0x0400.
//   4. the older rules do not read the new rule input.
#include <algorithm>
#include <cstdio>

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

static bool ok(const Scoring &sc, int lds_profile = 1000, int lds_tables = 1000) {
    return sym_affine_row_tables_ok(inputs(sc, 150, 64), 150, 64, 160, 10, lds_profile, lds_tables);
}

int main() {
    // 1. the largest byte: match' + (o - x) = match + 2x + o - x = match + o + x
    CHECK(sym_affine_row_table_high(aff(2, -1, -5, -1)) == 2 + 5 + 1 && sym_affine_row_table_low(aff(2, -1, -5, -1)) == 1);
    CHECK(ok(aff(2, -1, -5, -1)));
    for (int open = -5; open >= -40; open -= 7) {
        for (int ext = 0; ext >= open && ext >= -6; --ext) {
            const int o = -open, x = -ext;
            const int edge = 255 - o - x;                          // the match score whose row-0 byte is exactly 255
            const Scoring last = aff(edge, -x, open, ext), first = aff(edge + 1, -x, open, ext);
            if (!sym_affine_tilt_ok(inputs(first, 150, 64), 150, 64, 160, 10)) continue;
            CHECK(sym_affine_row_table_high(last) == 255 && ok(last));
            CHECK(sym_affine_row_table_high(first) == 256 && !ok(first));
            // a positive mismatch score is the largest byte where it exceeds the match score
            CHECK(ok(aff(1, edge, open, ext)) && !ok(aff(1, edge + 1, open, ext)));
            // the smallest byte: mismatch' = 0 / -1, match' = 0 / -1
            CHECK(sym_affine_row_table_low(aff(2, -2 * x, open, ext)) == 0 && ok(aff(2, -2 * x, open, ext)));
            CHECK(sym_affine_row_table_low(aff(2, -2 * x - 1, open, ext)) == -1 && !ok(aff(2, -2 * x - 1, open, ext)));
            CHECK(ok(aff(-2 * x, 3, open, ext)) && !ok(aff(-2 * x - 1, 3, open, ext)));
        }
    }
    CHECK(ok(aff(2, -2, -5, -1)) && !ok(aff(2, -3, -5, -1)));                     // mismatch' = 0 / -1 at x = 1
    CHECK(ok(aff(2, -1, -1, -1)) && ok(aff(2, 0, 0, 0)));                         // o - x = 0
    CHECK(!ok(aff(2, -1, -2, -3)));                                               // o - x < 0: the tables add it byte-wise

    // 2. what else refuses
    {
        const Scoring sc = aff(2, -1, -5, -1);
        RuleInputs in = inputs(sc, 150, 64);
        CHECK(sym_affine_row_tables_ok(in, 150, 64, 160, 10, 1000, 1000) && sym_affine_row_tables_ok(in, 150, 64, 160, 10, 1000, 16));
        CHECK(!sym_affine_row_tables_ok(in, 150, 64, 160, 10, 1000, 1001));      // more LDS than the plan's
        CHECK(!sym_affine_row_tables_ok(in, 150, 64, 1024, 16, 1000, 1000));     // K > kTiltMaxK: no tilted frame
        in.no_row_tables = true;
        CHECK(!sym_affine_row_tables_ok(in, 150, 64, 160, 10, 1000, 1000) && sym_affine_tilt_ok(in, 150, 64, 160, 10));
        in.no_row_tables = false;
        in.no_tilt = true;
        CHECK(!sym_affine_row_tables_ok(in, 150, 64, 160, 10, 1000, 1000));
        in.no_tilt = false;
        in.no_max3 = true;
        CHECK(!sym_affine_row_tables_ok(in, 150, 64, 160, 10, 1000, 1000));
        // beyond the tilted window (the match score of tests/sym_affine_tilt_rules_check.cpp's edge and one more)
        const Scoring big = aff(200, -1, -5, -1);
        CHECK(sym_affine_tilt_ok(inputs(big, 150, 64), 150, 64, 160, 10) == ok(big));
        CHECK(!ok(aff(480, -1, -5, -1)));
    }

    // 3. the window of a column that scores 0, over every scoring the rule accepts
    long long accepted = 0;
    for (int m = -3; m <= 40; ++m)
        for (int mm = -12; mm <= 6; ++mm)
            for (int open = 0; open >= -30; --open)
                for (int ext = 0; ext >= -6; --ext) {
                    const Scoring sc = aff(m, mm, open, ext);
                    if (!ok(sc)) continue;
                    ++accepted;
                    const int o = -open, x = -ext, B = sym_affine_tilt_bias(sc);
                    CHECK(x >= 0 && o - x >= 0);
                    CHECK(B + 3 * x - 2 * x >= kMax3WindowLow);                  // rows 1 .. K-1, u >= 3
                    CHECK(B + 2 * x - o - x >= kMax3WindowLow);                  // row 0, u >= 2
                    CHECK(std::min({m, mm, 0}) + 2 * x >= 0 && std::max({m, mm, 0}) + o + x <= 255);
                }
    CHECK(accepted > 1000);

    // 4. the older rules answer as before whatever the switch says
    {
        RuleInputs in = inputs(aff(2, -1, -5, -1), 150, 500);
        const bool tilt = sym_affine_tilt_ok(in, 150, 500, 160, 10), max3 = sym_affine_max3_ok(in, 150, 500);
        in.no_row_tables = true;
        CHECK(tilt && max3 && sym_affine_tilt_ok(in, 150, 500, 160, 10) == tilt && sym_affine_max3_ok(in, 150, 500) == max3);
        CHECK(std::string(ran_sym_affine_scores_name(true)) == "row_tables" && std::string(ran_sym_affine_scores_name(false)) == "lds_profile");
    }

    if (failures) {
        printf("%d check(s) FAILED\n", failures);
        return 1;
    }
    printf("sym affine row tables rules ok (%lld scorings accepted in the window walk)\n", accepted);
    return 0;
}
