// sym_affine_tilt_rules_check.cpp -- the rule behind the TILTED biased form of the int16 symmetric affine Smith-Waterman sweep
// (versalignlib_amd/csrc/cell_rules.h: sym_affine_tilt_bias / sym_affine_tilt_ok), on the CPU: plain g++, no HIP.
//   1. sym_affine_tilt_bias is 1024 + max(o - x, m) for the scorings of the sibling check (sym_affine_max3_rules_check.cpp).
//   2. sym_affine_tilt_ok flips exactly where B + x * (rows + F - lead) + hi passes 0x7BFF, the edge being computed here from
//      the sweep's own geometry (lane l, row q, step t: u = l (K - 1) + q + t + 2, steps = F + G - 1 - lead), not from the
//      rule's closed form; it is false for K = 16 and beyond, with no_tilt, with no_max3, and wherever sym_affine_max3_ok is.
//   3. sym_affine_bias and sym_affine_max3_ok do not read the new rule input and answer as before.
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

// the largest u of the sweep, walked: the last lane's last row at the last step
static long long walked_top_index(int R, int F, int G, int K) {
    const int rows = G * K;
    const int lead = rows > R ? (rows - R) / K : 0;
    const int steps = F + G - 1 - lead;
    long long top = 0;
    for (int l = 0; l < G; ++l) {
        const long long u = (long long)l * (K - 1) + (K - 1) + (steps - 1) + 2;
        top = u > top ? u : top;
    }
    return top;
}

int main() {
    // 1. the bias
    CHECK(sym_affine_tilt_bias(aff(2, -1, -5, -1)) == 1024 + 4);           // o - x = 4 > m = 1
    CHECK(sym_affine_tilt_bias(aff(2, 1, -5, -1)) == 1024 + 4);
    CHECK(sym_affine_tilt_bias(aff(5, -4, 0, 0)) == 1024 + 4);             // m alone
    CHECK(sym_affine_tilt_bias(aff(-2, -1, -4, 0)) == 1024 + 4);           // o - x = 4, m = 2 (a negative match score)
    CHECK(sym_affine_tilt_bias(aff(2, -1, -2, -3)) == 1024 + 1);           // an extension dearer than the opening: o - x < 0
    CHECK(sym_affine_tilt_bias(aff(2, 1, -1, -1)) == 1024);
    CHECK(sym_affine_tilt_bias(aff(479, -1, -5, -1)) == 1028);

    // 2. the rule's edge, on the geometries the form is built for
    struct { int G, K; } geos[] = {{16, 10}, {8, 12}, {32, 8}, {16, 8}, {64, 4}, {8, 10}};
    long long asked = 0;
    for (auto g : geos)
        for (int open = 0; open >= -40; open -= 5)
            for (int ext = 0; ext >= open && ext >= -6; --ext)
                for (int mm : {-7, -1, 0, 3})
                    for (int R : {1, 37, 64, 150}) {
                        const int rows = g.G * g.K;
                        if (R > rows) continue;
                        const int F = 64, len = std::min(R, F), x = -ext;
                        const int B = 1024 + std::max(-open - x, std::max(0, -mm));
                        const long long top = walked_top_index(R, F, g.G, g.K);
                        CHECK(top == sym_affine_tilt_top_index(R, F, rows, g.K));
                        const int last = (int)((0x7BFF - B - x * top - 1) / len);      // B + x * top + len * match + 1 <= 0x7BFF
                        CHECK(last > 3);
                        for (int match = last - 2; match <= last + 2; ++match) {
                            const Scoring sc = aff(match, mm, open, ext);
                            const RuleInputs in = inputs(sc, R, F);
                            // (a small extension: the tilted bias is the smaller one and its edge may lie beyond the plain
                            // form's, which bounds the tilted form too)
                            const bool plain = 1024 + -open + x + std::max(0, -mm) + (long long)len * match + 1 <= 0x7BFF;
                            const bool expect = match <= last && plain;
                            CHECK(sym_affine_max3_ok(in, R, F) == plain);
                            CHECK(sym_affine_tilt_ok(in, R, F, rows, g.K) == expect);
                            CHECK(!sym_affine_tilt_ok(in, R, F, 64 * 16, 16));        // K = 16, 24, 32 keep the plain frame
                            CHECK(!sym_affine_tilt_ok(in, R, F, 32 * 24, 24));
                            RuleInputs off = in;
                            off.no_tilt = true;
                            CHECK(!sym_affine_tilt_ok(off, R, F, rows, g.K));
                            CHECK(sym_affine_max3_ok(off, R, F) == sym_affine_max3_ok(in, R, F));      // (3.)
                            off = in;
                            off.no_max3 = true;
                            CHECK(!sym_affine_tilt_ok(off, R, F, rows, g.K));
                            ++asked;
                        }
                    }
    {
        // the cases of tests/test_gpu_sym_affine_tilted.py: 150 x 64 on 16 x 10, open -5, extend -1, mismatch -1 -- B = 1028,
        // lead 1, u <= 223: 1028 + 223 + 64 * 476 + 1 = 31 716, 477: 31 780 > 31 743
        CHECK(sym_affine_tilt_top_index(150, 64, 160, 10) == 223);
        CHECK(sym_affine_tilt_ok(inputs(aff(476, -1, -5, -1), 150, 64), 150, 64, 160, 10));
        CHECK(!sym_affine_tilt_ok(inputs(aff(477, -1, -5, -1), 150, 64), 150, 64, 160, 10));
        CHECK(sym_affine_max3_ok(inputs(aff(477, -1, -5, -1), 150, 64), 150, 64));
        // the headline shape
        CHECK(sym_affine_tilt_ok(inputs(aff(2, -1, -5, -1), 150, 500), 150, 500, 160, 10));
        CHECK(!sym_affine_tilt_ok(inputs(aff(2, -1, -5, -1), 150, 500), 150, 500, 64 * 16, 16));
        CHECK(sym_affine_tilt_ok(inputs(aff(2, -1, -5, -1), 150, 500), 150, 500, 96 * 2, 12));       // K = 12: the last tilted K
        CHECK(!sym_affine_tilt_ok(inputs(aff(2, -1, -5, -1), 150, 500), 150, 500, 14 * 16, 14));
        // a large extension: the tilt alone fills the window
        CHECK(sym_affine_tilt_ok(inputs(aff(2, -1, -50, -40), 150, 500), 150, 500, 160, 10));        // 1034 + 40 * 659 + 301
        CHECK(!sym_affine_tilt_ok(inputs(aff(2, -1, -50, -47), 150, 500), 150, 500, 160, 10));       // 1027 + 47 * 659 + 301 > 31 743
        CHECK(sym_affine_max3_ok(inputs(aff(2, -1, -50, -47), 150, 500), 150, 500));
        // not symmetric, not affine, positive gap scores: as the plain form
        Scoring sc = aff(2, -1, -5, -1);
        sc.open_read = -6;
        CHECK(!sym_affine_tilt_ok(inputs(sc, 150, 500), 150, 500, 160, 10));
        sc = aff(2, -1, -5, -1);
        sc.affine = false;
        CHECK(!sym_affine_tilt_ok(inputs(sc, 150, 500), 150, 500, 160, 10));
        CHECK(!sym_affine_tilt_ok(inputs(aff(2, -1, 1, 1), 150, 500), 150, 500, 160, 10));
        CHECK(!strcmp(ran_sym_affine_frame_name(true), "tilted") && !strcmp(ran_sym_affine_frame_name(false), "plain"));
    }

    // 3. the two older functions, value for value (the figures of sym_affine_max3_rules_check.cpp)
    CHECK(sym_affine_bias(aff(2, -1, -5, -1)) == 1024 + 5 + 1 + 1);
    CHECK(sym_affine_bias(aff(2, 1, -5, -1)) == 1024 + 5 + 1);
    CHECK(sym_affine_bias(aff(5, -4, 0, 0)) == 1024 + 4);
    CHECK(sym_affine_bias(aff(-2, -1, -4, 0)) == 1024 + 4 + 2);
    CHECK(sym_affine_max3_ok(inputs(aff(479, -1, -5, -1), 150, 64), 150, 64));
    CHECK(!sym_affine_max3_ok(inputs(aff(480, -1, -5, -1), 150, 64), 150, 64));
    CHECK(sym_affine_max3_ok(inputs(aff(2, -24, -600, -400), 150, 64), 150, 64));
    CHECK(!sym_affine_max3_ok(inputs(aff(2, -25, -600, -400), 150, 64), 150, 64));
    CHECK(asked > 5000);

    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("sym affine tilt rules ok (%lld rule comparisons)\n", asked);
    return 0;
}
