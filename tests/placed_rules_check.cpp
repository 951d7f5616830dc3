// placed_rules_check.cpp -- CPU check of placed_choice (versalignlib_amd/csrc/cell_rules.h; plain g++, no HIP;
// tests/test_placed_rules.py builds and runs it): what a placed-score call is.
//   1. the lane key at its edge: for K = 4, 10, 16 the largest min(R, F) * match that still takes the key -- found by walking,
//      compared with the rule's own inequality ((value + 1) << placed_key_bits(K) <= 32000) -- and that value + 1 takes the
//      per-row form; K = 24 and 32 never take the key;
//   2. every refusal, with its reason: the NW variant, a band, traceback_policy = 1, score_width = 32, cells that leave int16;
//      opt values above 1 are the caller's no-op and never reach the rule;
//   3. the strip threshold on both sides (1 024 / 1 025 rows), a forced geometry staying on the register path, and the
//      long-read plan taking the strips whatever the read.
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

// the largest top = min(R, F) * match (match = 1, F = 20000: top = R) that takes the key on K rows per lane; exactly one change
int key_edge(int K) {
    int edge = -1, changes = 0;
    bool prev = placed_choice(inputs(lin(1, -1, -3, -3), 1, 20000), kAlgSW, PlacedFacts{0, 0, true, false}, 64, K).route == PlacedRoute::Key;
    for (int top = 2; top <= 12000; ++top) {
        const PlacedChoice c = placed_choice(inputs(lin(1, -1, -3, -3), top, 20000), kAlgSW, PlacedFacts{0, 0, true, false}, 64, K);
        expect(c.route == PlacedRoute::Key || c.route == PlacedRoute::Rows, "a forced register geometry runs key or rows");
        const bool key = c.route == PlacedRoute::Key;
        if (key) expect(c.key_bits == placed_key_bits(K), "the choice carries the key's bits");
        if (key != prev) {
            ++changes;
            edge = top - 1;
        }
        prev = key;
    }
    expect(changes <= 1, "at most one change from key to rows");
    return changes == 1 ? edge : (prev ? 12000 : 0);
}

}  // namespace

int main() {
    // ---- 1. the key's edge ----
    expect(placed_key_bits(4) == 2 && placed_key_bits(6) == 3 && placed_key_bits(8) == 3 && placed_key_bits(10) == 4 &&
               placed_key_bits(12) == 4 && placed_key_bits(16) == 4,
           "bits for the rows of a lane");
    for (int K : {4, 10, 16}) {
        const int bits = placed_key_bits(K);
        expect((1 << bits) >= K, "the key's bits hold the lane's rows");
        const int edge = key_edge(K);
        const int by_formula = 32000 / (1 << bits) - 1;           // (top + 1) << bits <= 32000
        expect(edge == by_formula, "K = " + std::to_string(K) + ": last top inside " + std::to_string(edge) + ", formula " + std::to_string(by_formula));
        // the same edge reached through match: min(R, F) = 100
        for (int match = 1; match <= 200; ++match) {
            const bool key = placed_choice(inputs(lin(match, -1, -3, -3), 100, 300), kAlgSW, PlacedFacts{}, 64, K).route == PlacedRoute::Key;
            expect(key == (100 * match <= by_formula), "K = " + std::to_string(K) + ", match " + std::to_string(match));
        }
        // the largest key stays inside int16
        expect((((long long)edge << bits) | ((1 << bits) - 1)) <= 32767, "the largest key is a short");
    }
    expect(key_edge(4) == 7999 && key_edge(10) == 1999 && key_edge(16) == 1999, "the edges as documented");
    for (int K : {24, 32})
        for (int top : {1, 10, 100, 1000})
            expect(placed_choice(inputs(lin(1, -1, -3, -3), top, 4000), kAlgSW, PlacedFacts{0, 0, true, false}, 64, K).route == PlacedRoute::Rows,
                   "more than 16 rows per lane: per row");
    // affine scorings read the same bound
    expect(placed_choice(inputs(aff(13, -1, -5, -1, -5, -1), 150, 500), kAlgSW, PlacedFacts{}, 16, 10).route == PlacedRoute::Key, "150 x 13 = 1950: key");
    expect(placed_choice(inputs(aff(14, -1, -5, -1, -5, -1), 150, 500), kAlgSW, PlacedFacts{}, 16, 10).route == PlacedRoute::Rows, "150 x 14 = 2100: rows");

    // ---- 2. refusals ----
    const RuleInputs plain = inputs(lin(2, -1, -3, -3), 150, 500);
    auto refused = [&](const RuleInputs &in, int alg, const PlacedFacts &f, const char *word) {
        const PlacedChoice c = placed_choice(in, alg, f, 16, 10);
        expect(c.route == PlacedRoute::Refused && strstr(c.reason, word) != nullptr, std::string("refused with '") + word + "': " + c.reason);
    };
    expect(placed_choice(plain, kAlgSW, PlacedFacts{}, 16, 10).route == PlacedRoute::Key, "the plain call runs");
    expect(placed_choice(plain, kAlgSW, PlacedFacts{}, 16, 10).reason[0] == 0, "... without a reason");
    refused(plain, kAlgNW, PlacedFacts{}, "Smith-Waterman only");
    refused(plain, kAlgSW, PlacedFacts{64, 0, false, false}, "band_width");
    RuleInputs sse = plain;
    sse.sse_policy = true;
    refused(sse, kAlgSW, PlacedFacts{}, "traceback_policy");
    refused(plain, kAlgSW, PlacedFacts{0, 32, false, false}, "score_width");
    expect(placed_choice(plain, kAlgSW, PlacedFacts{0, 16, false, false}, 16, 10).route == PlacedRoute::Key, "score_width = 16 is what placed scores run on");
    // cells that could leave int16: the rule of the score path, at its edge (min(R, F) * match + 1 <= 32000)
    expect(placed_choice(inputs(lin(213, -1, -3, -3), 150, 500), kAlgSW, PlacedFacts{}, 16, 10).route == PlacedRoute::Rows, "150 x 213 = 31950: int16");
    refused(inputs(lin(214, -1, -3, -3), 150, 500), kAlgSW, PlacedFacts{}, "int16");
    refused(inputs(lin(2, -32001, -3, -3), 150, 500), kAlgSW, PlacedFacts{}, "int16");
    for (int m = 200; m <= 220; ++m) {
        const RuleInputs in = inputs(lin(m, -1, -3, -3), 150, 500);
        expect((placed_choice(in, kAlgSW, PlacedFacts{}, 16, 10).route == PlacedRoute::Refused) == !int16_range_ok(in, kAlgSW, true, false, 0),
               "the int16 refusal is int16_range_ok's");
    }
    // the refusals come before the route: a long read under a band is refused, not stripped
    refused(inputs(lin(2, -1, -3, -3), 5000, 5000), kAlgSW, PlacedFacts{64, 0, false, false}, "band_width");

    // ---- 3. strips ----
    expect(kPlacedStripRows == 1024, "the threshold alignments use");
    expect(placed_choice(inputs(lin(2, -1, -3, -3), 1024, 1300), kAlgSW, PlacedFacts{}, 64, 16).route != PlacedRoute::Strip, "1 024 rows: a register sweep");
    expect(placed_choice(inputs(lin(2, -1, -3, -3), 1024, 1300), kAlgSW, PlacedFacts{}, 64, 16).route == PlacedRoute::Rows, "... whose values leave the key");
    expect(placed_choice(inputs(lin(2, -1, -3, -3), 1025, 1300), kAlgSW, PlacedFacts{}, 64, 24).route == PlacedRoute::Strip, "1 025 rows: strips");
    expect(placed_choice(inputs(aff(2, -1, -5, -1, -5, -1), 1025, 1300), kAlgSW, PlacedFacts{}, 64, 24).route == PlacedRoute::Strip, "... affine too");
    expect(placed_choice(inputs(lin(2, -1, -3, -3), 1025, 1300), kAlgSW, PlacedFacts{0, 0, true, false}, 64, 24).route == PlacedRoute::Rows,
           "a forced geometry stays on the register path");
    expect(placed_choice(inputs(lin(2, -1, -3, -3), 150, 20000), kAlgSW, PlacedFacts{0, 0, false, true}, 16, 10).route == PlacedRoute::Strip,
           "the long-read plan: strips whatever the read");
    expect(placed_choice(inputs(lin(2, -1, -3, -3), 10000, 10000), kAlgSW, PlacedFacts{0, 0, false, true}, 16, 10).key_bits == 0, "strips carry no key");
    expect(!strcmp(ran_placed_name(PlacedRoute::Refused), "none") && !strcmp(ran_placed_name(PlacedRoute::Key), "key") &&
               !strcmp(ran_placed_name(PlacedRoute::Rows), "rows") && !strcmp(ran_placed_name(PlacedRoute::Strip), "strip"),
           "describe()'s names");

    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("placed rules ok\n");
    return 0;
}
