// sym_affine_max3_rules_check.cpp -- the rule behind the biased three-operand-maximum form of the int16 symmetric affine
// Smith-Waterman sweep (versalignlib_amd/csrc/cell_rules.h: sym_affine_bias / sym_affine_max3_ok), on the CPU: plain g++, no HIP.
//   1. The window itself: for every bit pattern p in [0x0400, 0x7BFF] the half float of p is finite, positive, normal, and
//      smaller than the half float of p + 1 (0x7C00, +inf, ends the window) -- so a half-float maximum of such patterns is
//      their integer maximum.
//   2. sym_affine_bias is 1024 + o + x + m, and sym_affine_max3_ok flips exactly where B + hi passes 0x7BFF (hi as
//      int16_range_ok counts the largest cell, a positive mismatch score included), where o + x + m passes 1024, with the
//      debug switch, and for scorings that are not symmetric affine.
//   3. score_gap_form, int16_range_ok and gap_form_f16 do not read the new rule input.
#include <cmath>
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

// the value of a half-float bit pattern, decoded by hand (no compiler support for _Float16 needed)
static double half_value(unsigned p) {
    const int sign = (p >> 15) & 1, exp = (p >> 10) & 31, man = p & 1023;
    double v;
    if (exp == 31) v = man ? NAN : INFINITY;
    else if (exp == 0) v = std::ldexp((double)man, -24);
    else v = std::ldexp(1024.0 + man, exp - 25);
    return sign ? -v : v;
}

static Scoring aff(int m, int mm, int open, int ext) { return Scoring{m, mm, -3, -3, true, open, ext, open, ext}; }

static RuleInputs inputs(const Scoring &sc, int R, int F) {
    RuleInputs in;
    in.sc = sc;
    in.R = R;
    in.F = F;
    return in;
}

int main() {
    // 1. the window
    CHECK(kMax3WindowLow == 0x0400 && kMax3WindowHigh == 0x7BFF);
    // (ordered they are from zero up, all 31,744 non-negative finite patterns; the window is the 30,720 normal ones of them)
    int patterns = 0, in_window = 0;
    for (unsigned p = 0; p <= (unsigned)kMax3WindowHigh; ++p, ++patterns) {
        const double v = half_value(p), next = half_value(p + 1);
        CHECK(std::isfinite(v) && v < next);                           // (p + 1 = 0x7C00: +inf)
        if (p >= (unsigned)kMax3WindowLow) {
            CHECK(v >= std::ldexp(1.0, -14));                          // positive and normal
            ++in_window;
        }
    }
    CHECK(patterns == 31744 && in_window == 30720);
    CHECK(half_value(0x03FF) < std::ldexp(1.0, -14));                  // below the window: a denormal
    CHECK(std::isinf(half_value(0x7C00)));                             // above it: +inf, then NaNs

    // 2. the bias and the rule's edges
    CHECK(sym_affine_bias(aff(2, -1, -5, -1)) == 1024 + 5 + 1 + 1);
    CHECK(sym_affine_bias(aff(2, 1, -5, -1)) == 1024 + 5 + 1);          // a positive mismatch score takes nothing off a cell
    CHECK(sym_affine_bias(aff(5, -4, 0, 0)) == 1024 + 4);
    CHECK(sym_affine_bias(aff(-2, -1, -4, 0)) == 1024 + 4 + 2);         // ... a negative match score does
    for (int open = 0; open >= -40; open -= 5)
        for (int ext = 0; ext >= open; --ext)
            for (int mm : {-7, -1, 0, 3}) {
                for (int R : {1, 37, 64, 150}) {
                    const int F = 64, len = std::min(R, F);
                    const int B = 1024 + -open + -ext + std::max(0, -mm);
                    // the largest match score the window holds for this shape: B + len * match + 1 <= 0x7BFF
                    const int last = (0x7BFF - B - 1) / len;
                    CHECK(last > 3);
                    for (int match = last - 2; match <= last + 2; ++match) {
                        const Scoring sc = aff(match, mm, open, ext);
                        const long long hi = (long long)len * std::max(match, std::max(mm, 0)) + 1;
                        const bool expect = B + hi <= 0x7BFF;
                        CHECK(expect == (match <= last));
                        CHECK(sym_affine_max3_ok(inputs(sc, R, F), R, F) == expect);
                        CHECK(sym_affine_max3_ok(inputs(sc, F, R), F, R) == expect);     // min(R, F)
                        RuleInputs off = inputs(sc, R, F);
                        off.no_max3 = true;
                        CHECK(!sym_affine_max3_ok(off, R, F));
                    }
                }
            }
    {
        // the cases of tests/test_gpu_sym_affine_max3.py: 150 x 64, open -5, extend -1, mismatch -1 -- B = 1031
        CHECK(sym_affine_bias(aff(479, -1, -5, -1)) == 1031);
        CHECK(sym_affine_max3_ok(inputs(aff(479, -1, -5, -1), 150, 64), 150, 64));        // 1031 + 30 657 = 31 688
        CHECK(!sym_affine_max3_ok(inputs(aff(480, -1, -5, -1), 150, 64), 150, 64));       // 1031 + 30 721 = 31 752
        CHECK(!sym_affine_max3_ok(inputs(aff(499, -1, -5, -1), 150, 64), 150, 64));
        CHECK(int16_range_ok(inputs(aff(499, -1, -5, -1), 150, 64), kAlgSW, true, false, 0));   // the last int16 value: 31 937
        CHECK(!int16_range_ok(inputs(aff(500, -1, -5, -1), 150, 64), kAlgSW, true, false, 0));
        // a positive mismatch score larger than the match score bounds the cells
        CHECK(sym_affine_max3_ok(inputs(aff(1, 479, -5, -1), 150, 64), 150, 64));
        CHECK(!sym_affine_max3_ok(inputs(aff(1, 480, -5, -1), 150, 64), 150, 64));
        // o + x + m <= 1024
        CHECK(sym_affine_max3_ok(inputs(aff(2, -24, -600, -400), 150, 64), 150, 64));
        CHECK(!sym_affine_max3_ok(inputs(aff(2, -25, -600, -400), 150, 64), 150, 64));
        // not symmetric, not affine, positive gap scores
        Scoring sc = aff(2, -1, -5, -1);
        CHECK(sym_affine_max3_ok(inputs(sc, 150, 500), 150, 500));
        sc.open_read = -6;
        CHECK(!sym_affine_max3_ok(inputs(sc, 150, 500), 150, 500));
        sc = aff(2, -1, -5, -1);
        sc.ext_read = 0;
        CHECK(!sym_affine_max3_ok(inputs(sc, 150, 500), 150, 500));
        sc = aff(2, -1, -5, -1);
        sc.affine = false;
        CHECK(!sym_affine_max3_ok(inputs(sc, 150, 500), 150, 500));
        CHECK(!sym_affine_max3_ok(inputs(aff(2, -1, 1, 1), 150, 500), 150, 500));
        CHECK(!strcmp(ran_sym_affine_name(true), "max3") && !strcmp(ran_sym_affine_name(false), "sources"));
    }

    // 3. the older rules do not read the new input
    long long asked = 0;
    for (int alg : {kAlgSW, kAlgNW})
        for (int match : {1, 2, 13, 200, 479, 480})
            for (int open : {0, -1, -5})
                for (int ext : {0, -1})
                    for (bool affine : {false, true})
                        for (bool sym : {false, true})
                            for (bool no_f16 : {false, true})
                                for (int R : {10, 150, 1500})
                                    for (int F : {7, 64, 500}) {
                                        Scoring sc = aff(match, -1, open, ext);
                                        sc.affine = affine;
                                        if (!sym) sc.open_read -= 1, sc.gap_read -= 1;
                                        RuleInputs a = inputs(sc, R, F), b = a;
                                        a.no_f16 = b.no_f16 = no_f16;
                                        b.no_max3 = true;
                                        for (int rows : {160, 256}) {
                                            const int fa = score_gap_form(a, alg, R, F, rows), fb = score_gap_form(b, alg, R, F, rows);
                                            CHECK(fa == fb && gap_form_f16(fa) == gap_form_f16(fb));
                                            CHECK(int16_range_ok(a, alg, true, false, rows) == int16_range_ok(b, alg, true, false, rows));
                                            ++asked;
                                        }
                                    }
    CHECK(asked > 5000);

    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("sym affine max3 rules ok (%d window patterns, %lld rule comparisons)\n", patterns, asked);
    return 0;
}
