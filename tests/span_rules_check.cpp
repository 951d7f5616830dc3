// span_rules_check.cpp -- CPU check of span_ref_length and span_choice (versalignlib_amd/csrc/cell_rules.h; plain g++, no HIP;
// tests/test_span_rules.py builds and runs it): how far the reverse sweep of a spanned call looks back, and what such a call
// refuses.
//   1. span_ref_length against its formula restated here, the worked values of the header, and its edges: c = 0, match <= 0,
//      mismatch > match, Fr exactly F and F +- 1, affine with |open| < |ext|, the largest shape int32_refused admits;
//   2. span_choice: every refusal of an unbanded placed call with placed_choice's own text, the band refusal with and without
//      band_placed, and the routes of a call that runs.
#include "cell_rules.h"

#include <stdio.h>
#include <string.h>

using namespace valign;

namespace {

int failures = 0;
void expect(bool ok, const std::string &what) {
    if (!ok && ++failures <= 20) fprintf(stderr, "FAIL: %s\n", what.c_str());
}

Scoring lin(int m, int mm, int gr, int gf) { return Scoring{m, mm, gr, gf, false, gr, gr, gf, gf}; }
Scoring aff(int m, int mm, int orr, int er, int of, int ef) { return Scoring{m, mm, orr, of, true, orr, er, of, ef}; }

RuleInputs inputs(const Scoring &sc, int R, int F) {
    RuleInputs in;
    in.sc = sc;
    in.R = R;
    in.F = F;
    return in;
}

long long fr(const Scoring &sc, int R, int F) { return span_ref_length(inputs(sc, R, F)); }

}  // namespace

int main() {
    // ---- 1. the bound ----
    expect(fr(lin(2, -1, -3, -3), 20, 120) == 33, "20 x 120, -3 / -3, match 2: 33");
    expect(fr(lin(2, -1, -3, -3), 150, 500) == 249, "150 x 500 linear -3: 249");
    expect(fr(aff(2, -1, -5, -1, -5, -1), 150, 500) == 449, "150 x 500 affine, extend -1: 449");
    expect(fr(lin(2, -1, -3, -3), 150, 2000) == 249 && fr(lin(2, -1, -3, -3), 150, 8000) == 249, "the bound does not grow with F");
    // only the price of a gap in the READ counts (a reference base against a gap)
    expect(fr(lin(2, -1, -3, -1), 20, 120) == 33 && fr(lin(2, -1, -1, -3), 20, 120) == 59, "gap_read, not gap_ref");
    // c = 0: no bound
    expect(fr(lin(2, -1, 0, -3), 20, 120) == 120, "gap_read = 0: F");
    expect(fr(aff(2, -1, -5, 0, -5, -1), 20, 120) == 120, "ext_read = 0: F");
    expect(fr(aff(2, -1, -5, -1, -5, 0), 20, 120) == 20 + 39, "ext_ref = 0 is not read");
    // match <= 0: nothing scores; the diagonals alone
    expect(fr(lin(0, -1, -3, -3), 20, 120) == 20 && fr(lin(-2, -3, -3, -3), 20, 120) == 20, "match <= 0: R");
    expect(fr(lin(0, -1, -3, -3), 20, 9) == 9 && fr(lin(0, 0, -3, -3), 0, 9) == 0, "... or F, and never negative");
    // mismatch > match: the larger of the two is what a diagonal column can give
    expect(fr(lin(1, 4, -3, -3), 20, 120) == 20 + 79 / 3, "mismatch 4 > match 1: m = 4");
    expect(fr(lin(-1, 3, -2, -3), 10, 500) == 10 + 29 / 2, "match < 0 < mismatch");
    // Fr exactly F, F - 1, F + 1 (R = 20, m = 2, c = 3: R + 13 = 33)
    expect(fr(lin(2, -1, -3, -3), 20, 33) == 33 && fr(lin(2, -1, -3, -3), 20, 32) == 32 && fr(lin(2, -1, -3, -3), 20, 34) == 33, "F = 33, 32, 34");
    // the floor: (R m - 1) / c at a multiple of c and one beside it (R = 3, m = 2: 5 / c)
    expect(fr(lin(2, -1, -5, -5), 3, 100) == 4 && fr(lin(2, -1, -6, -6), 3, 100) == 3 && fr(lin(2, -1, -1, -1), 3, 100) == 8, "floor((R m - 1) / c)");
    // affine: the cheaper of opening and extension, whichever it is (the engine refuses |open| < |ext|; the rule stays safe there)
    expect(fr(aff(2, -1, -1, -4, -5, -1), 20, 500) == 20 + 39, "|open_read| < |ext_read|: c = |open_read|");
    expect(fr(aff(2, -1, -4, -2, -5, -1), 20, 500) == 20 + 19, "|ext_read| < |open_read|: c = |ext_read|");
    // every value against the formula, restated
    for (int R : {1, 2, 7, 150, 1000})
        for (int F : {1, 9, 151, 4000})
            for (int m : {-1, 0, 1, 2, 7})
                for (int c : {0, 1, 2, 3, 11}) {
                    const long long got = fr(lin(m, -1, -c, -3), R, F);
                    const long long mm = m > 0 ? m : 0;
                    const long long exp = c == 0 ? F : std::min<long long>(F, R + (R * mm >= 1 ? (R * mm - 1) / c : 0));
                    expect(got == exp && got >= 0 && got <= F, "formula at R " + std::to_string(R) + " F " + std::to_string(F) + " m " + std::to_string(m) + " c " + std::to_string(c));
                }
    // the largest shape int32_refused admits: R + F = 32766 rows and columns of the ABI at the largest scores it lets through --
    // (R + F + 2) * worst < 2^28 -> worst = 8191; long long arithmetic, no overflow
    {
        const Scoring big = lin(8191, -8191, -1, -8191);
        const RuleInputs in = inputs(big, 16383, 16383);
        expect(!int32_refused(in), "8191 at 16383 x 16383 is admitted");
        expect(int32_refused(inputs(lin(8192, -1, -1, -1), 16383, 16383)), "... and 8192 is not");
        expect(span_ref_length(in) == 16383, "clipped to F");
        expect(span_ref_length(inputs(big, 16383, 2000000000)) == 16383ll + (16383ll * 8191 - 1), "R m - 1 columns of gaps, exact");
        expect(span_ref_length(inputs(lin(32767, -1, -1, -1), 2000000000, 2000000000)) == 2000000000ll, "R m beyond int32: no overflow");
    }

    // ---- 2. refusals ----
    const RuleInputs plain = inputs(lin(2, -1, -3, -3), 150, 500);
    auto refused = [&](const RuleInputs &in, int alg, const PlacedFacts &f, const char *word) {
        const PlacedChoice c = span_choice(in, alg, f, 16, 10);
        expect(c.route == PlacedRoute::Refused && strstr(c.reason, word) != nullptr, std::string("refused with '") + word + "': " + c.reason);
        PlacedFacts unbanded = f;
        unbanded.band_width = 0;
        const PlacedChoice p = placed_choice(in, alg, unbanded, 16, 10);
        if (p.route == PlacedRoute::Refused) expect(!strcmp(p.reason, c.reason), std::string("placed_choice's own text: ") + c.reason);
    };
    expect(span_choice(plain, kAlgSW, PlacedFacts{}, 16, 10).route == PlacedRoute::Key, "the plain call runs, on the forward sweep's route");
    expect(span_choice(plain, kAlgSW, PlacedFacts{}, 16, 10).reason[0] == 0, "... without a reason");
    expect(span_choice(plain, kAlgSW, PlacedFacts{}).route != PlacedRoute::Refused, "... and without a geometry: not refused");
    expect(span_choice(inputs(lin(2, -1, -3, -3), 1025, 1300), kAlgSW, PlacedFacts{}, 64, 24).route == PlacedRoute::Strip, "1 025 rows: strips");
    refused(plain, kAlgNW, PlacedFacts{}, "Smith-Waterman only");
    RuleInputs sse = plain;
    sse.sse_policy = true;
    refused(sse, kAlgSW, PlacedFacts{}, "traceback_policy");
    refused(plain, kAlgSW, PlacedFacts{0, 32, false, false}, "score_width");
    refused(inputs(lin(214, -1, -3, -3), 150, 500), kAlgSW, PlacedFacts{}, "int16");
    expect(span_choice(inputs(lin(213, -1, -3, -3), 150, 500), kAlgSW, PlacedFacts{}, 16, 10).route == PlacedRoute::Rows, "150 x 213: inside int16");
    // the band: refused with and without band_placed, with a usable chain or not
    const char *band_text = "spanned scores are not built for band_width > 0";
    for (bool band_placed : {false, true})
        for (bool usable : {false, true}) {
            const PlacedChoice c = span_choice(plain, kAlgSW, PlacedFacts{64, 0, false, false, band_placed, usable}, 16, 10);
            expect(c.route == PlacedRoute::Refused && !strcmp(c.reason, band_text), std::string("band refused: ") + c.reason);
        }
    expect(placed_choice(plain, kAlgSW, PlacedFacts{64, 0, false, false, true, true}, 16, 10).route == PlacedRoute::Chain, "(placed scores do run there)");
    // what an unbanded call refuses is refused under a band with ITS text, first
    refused(plain, kAlgNW, PlacedFacts{64, 0, false, false, true, true}, "Smith-Waterman only");
    refused(sse, kAlgSW, PlacedFacts{64, 0, false, false, true, true}, "traceback_policy");
    refused(plain, kAlgSW, PlacedFacts{64, 32, false, false, true, true}, "score_width");
    refused(inputs(lin(2, -1, -3, -3), 5000, 5000), kAlgSW, PlacedFacts{64, 0, false, true, true, true}, "band_width");

    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("span rules ok\n");
    return 0;
}
