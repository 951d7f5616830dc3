// extend_rules_check.cpp -- CPU check of extend_choice (versalignlib_amd/csrc/cell_rules.h; plain g++, no HIP;
// tests/test_extend_rules.py builds and runs it, once more under ASan + UBSan): what an extension-score call refuses, with which
// text, and both sides of each edge of the signed int16 bound.
//   1. the route of a call that runs: Rows, whatever the geometry;
//   2. every refusal: the NW variant's mode bit, traceback_policy = 1, any band whatever band_placed says, score_width = 32
//      whatever placed_wide says, the row strips;
//   3. the bound: the top edge on match and on a positive mismatch, the bottom edge with linear and with affine gaps -- the
//      all-gaps path to the far corner plus the largest single addend -- each one step inside and one step outside.
// With arguments -- R F match mismatch gap_read gap_ref affine open_read ext_read open_ref ext_ref -- it prints the rule's answer
// and the bound's two ends for that shape x scoring instead (tests/test_extend_ref.py holds the restatement's cells against it).
#include "cell_rules.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace valign;

namespace {

int failures = 0;
void expect(bool ok, const std::string &what) {
    if (!ok && ++failures <= 20) fprintf(stderr, "FAIL: %s\n", what.c_str());
}

Scoring lin(int m, int mm, int gr, int gf) { return Scoring{m, mm, gr, gf, false, gr, gr, gf, gf}; }
Scoring aff(int m, int mm, int o_read, int e_read, int o_ref, int e_ref) { return Scoring{m, mm, -3, -3, true, o_read, e_read, o_ref, e_ref}; }

RuleInputs inputs(const Scoring &sc, int R, int F) {
    RuleInputs in;
    in.sc = sc;
    in.R = R;
    in.F = F;
    return in;
}

bool runs(const RuleInputs &in) { return extend_choice(in, kAlgSW, PlacedFacts{}, 16, 10).route == PlacedRoute::Rows; }
bool refused_for_range(const RuleInputs &in) {
    const PlacedChoice c = extend_choice(in, kAlgSW, PlacedFacts{}, 16, 10);
    return c.route == PlacedRoute::Refused && strstr(c.reason, "signed int16 cells") != nullptr;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 12) {
        int v[11];
        for (int i = 0; i < 11; ++i) v[i] = atoi(argv[i + 1]);
        const RuleInputs in = inputs(Scoring{v[2], v[3], v[4], v[5], v[6] != 0, v[7], v[8], v[9], v[10]}, v[0], v[1]);
        const PlacedChoice c = extend_choice(in, kAlgSW, PlacedFacts{}, 0, 0);
        printf("%s %lld %lld\n", c.route == PlacedRoute::Rows ? "accept" : "refuse", extend_cell_top(in), extend_cell_bottom(in));
        return 0;
    }
    const RuleInputs plain = inputs(lin(2, -1, -3, -3), 150, 500);
    // ---- 1. a call that runs ----
    for (int G : {8, 16, 32, 64})
        for (int K : {8, 10, 16, 32}) {
            const PlacedChoice c = extend_choice(plain, kAlgSW, PlacedFacts{}, G, K);
            expect(c.route == PlacedRoute::Rows && c.reason[0] == 0, "150 x 500 runs on the rows track, no reason");
        }
    expect(runs(inputs(aff(2, -1, -5, -1, -4, -2), 150, 500)), "affine gaps run");

    // ---- 2. the refusals ----
    auto refused = [&](const RuleInputs &in, int alg, const PlacedFacts &f, const char *word) {
        const PlacedChoice c = extend_choice(in, alg, f, 16, 10);
        expect(c.route == PlacedRoute::Refused && strstr(c.reason, word) != nullptr, std::string("refused with '") + word + "': " + c.reason);
    };
    refused(plain, kAlgNW, PlacedFacts{}, "opt & 0xF == 0 only");
    RuleInputs sse = plain;
    sse.sse_policy = true;
    refused(sse, kAlgSW, PlacedFacts{}, "traceback_policy = 1");
    for (bool band_placed : {false, true})
        for (bool usable : {false, true})
            refused(plain, kAlgSW, PlacedFacts{64, 0, false, false, band_placed, usable}, "not built for band_width > 0");
    expect(placed_choice(plain, kAlgSW, PlacedFacts{64, 0, false, false, true, true}, 16, 10).route == PlacedRoute::Chain, "(placed scores do run under band_placed)");
    for (bool wide : {false, true}) {
        PlacedFacts f{};
        f.placed_wide = wide;
        f.score_width = 32;
        refused(plain, kAlgSW, f, "score_width = 32");
        f.score_width = 16;
        expect(extend_choice(plain, kAlgSW, f, 16, 10).route == PlacedRoute::Rows, "score_width = 16 runs");
        f.score_width = 0;
        // placed_wide opens no int32 sweep here
        refused(inputs(lin(214, -1, -3, -3), 150, 500), kAlgSW, f, "signed int16 cells");
    }
    {
        const RuleInputs tall = inputs(lin(2, -1, -3, -3), 1025, 1300);
        refused(tall, kAlgSW, PlacedFacts{}, "register sweep only");
        expect(runs(inputs(lin(2, -1, -3, -3), 1024, 1300)), "1 024 rows run");
        expect(extend_choice(tall, kAlgSW, PlacedFacts{0, 0, true}, 64, 32).route == PlacedRoute::Rows, "a forced geometry stays on the register sweep");
        PlacedFacts lng{};
        lng.long_plan = true;
        refused(plain, kAlgSW, lng, "register sweep only");
        refused(inputs(lin(2, -1, -3, -3), 1500, 1500), kAlgSW, PlacedFacts{}, "register sweep only");
    }
    // the order: the mode bit first, the range before the strips
    refused(sse, kAlgNW, PlacedFacts{64, 32, false, true, false, false}, "opt & 0xF == 0 only");
    refused(inputs(lin(2, -1, -30, -30), 1500, 1500), kAlgSW, PlacedFacts{}, "signed int16 cells");

    // ---- 3. the bound, both sides of each edge ----
    // top: min(R, F) x max(match, mismatch, 0) <= 32000
    expect(runs(inputs(lin(213, -1, -3, -3), 150, 500)) && refused_for_range(inputs(lin(214, -1, -3, -3), 150, 500)), "150 x match 213 | 214");
    expect(runs(inputs(lin(320, -1, -3, -3), 100, 100)) && refused_for_range(inputs(lin(321, -1, -3, -3), 100, 100)), "100 x match 320 | 321: exactly 32000 runs");
    expect(runs(inputs(lin(213, -1, -3, -3), 500, 150)) && refused_for_range(inputs(lin(214, -1, -3, -3), 500, 150)), "the shorter side counts, whichever it is");
    expect(runs(inputs(lin(1, 320, -3, -3), 100, 100)) && refused_for_range(inputs(lin(1, 321, -3, -3), 100, 100)), "a positive mismatch above the match counts");
    expect(extend_cell_top(inputs(lin(-2, -5, -3, -3), 100, 100)) == 0, "no positive score: no cell above 0");
    // bottom, linear: R gap_ref + F gap_read + the largest single addend >= -32000
    expect(extend_cell_bottom(plain) == -3 * 150 - 3 * 500 - 3, "150 x 500 at -3 / -3: -1953");
    expect(runs(inputs(lin(2, -200, -159, -159), 100, 100)) && refused_for_range(inputs(lin(2, -201, -159, -159), 100, 100)),
           "200 steps at -159 and a mismatch of -200 | -201: exactly -32000 runs");
    expect(runs(inputs(lin(2, -1, -158, -160), 100, 100)) && refused_for_range(inputs(lin(2, -1, -159, -160), 100, 100)),
           "each direction at its own price, the addend the worse gap: -15800 - 16000 - 160 | -15900 - 16000 - 160");
    expect(runs(inputs(lin(2, -1, -49, -49), 150, 500)) && refused_for_range(inputs(lin(2, -1, -50, -50), 150, 500)), "150 x 500 at -49 | -50");
    // bottom, affine: every step at the worse of open and extend
    expect(extend_cell_bottom(inputs(aff(2, -1, -100, -1, -200, -1), 100, 100)) == -100 * 100 - 200 * 100 - 200, "affine: the openings price the steps");
    expect(runs(inputs(aff(2, -1, -100, -1, -217, -1), 100, 100)) && refused_for_range(inputs(aff(2, -1, -100, -1, -218, -1), 100, 100)),
           "open_ref -217 | -218: -31917 | -32018");
    expect(runs(inputs(aff(2, -300, -100, -1, -217, -1), 100, 100)) && refused_for_range(inputs(aff(2, -301, -100, -1, -217, -1), 100, 100)),
           "the addend is the mismatch where it is the largest: -32000 | -32001");
    // the affine model does not read the linear scores, nor the linear one the affine scores
    {
        Scoring sc = aff(2, -1, -5, -1, -5, -1);
        sc.gap_read = sc.gap_ref = -30000;
        expect(runs(inputs(sc, 150, 500)), "affine: gap_read / gap_ref are not read");
        Scoring l = lin(2, -1, -3, -3);
        l.open_read = l.open_ref = -30000;
        expect(runs(inputs(l, 150, 500)), "linear: the affine scores are not read");
    }

    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("extend rules ok\n");
    return 0;
}
