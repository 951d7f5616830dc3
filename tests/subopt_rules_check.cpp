// subopt_rules_check.cpp -- CPU check of subopt_choice (versalignlib_amd/csrc/cell_rules.h; plain g++, no HIP;
// tests/test_subopt_rules.py builds and runs it): what a suboptimal-score call refuses, with which text, and the two tracks of a
// call that runs.
//   1. both routes: Key where the lane key holds the largest value, Rows beyond it and for more than 16 rows per lane;
//   2. every refusal of an unbanded placed call with placed_choice's own text, placed_wide or not;
//   3. the refusals of its own: mask < 0, any band whatever band_placed says, the row strips;
//   4. subopt_block_waves: the waves of a block once every wave carries a ring, and the refusal where one wave cannot.
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

RuleInputs inputs(const Scoring &sc, int R, int F) {
    RuleInputs in;
    in.sc = sc;
    in.R = R;
    in.F = F;
    return in;
}

}  // namespace

int main() {
    const RuleInputs plain = inputs(lin(2, -1, -3, -3), 150, 500);
    // ---- 1. the routes ----
    {
        const PlacedChoice c = subopt_choice(plain, kAlgSW, PlacedFacts{}, 16, 10, 75);
        expect(c.route == PlacedRoute::Key && c.key_bits == 4 && c.reason[0] == 0, "150 x 500 on 16 x 10: the key, 4 bits, no reason");
    }
    expect(subopt_choice(plain, kAlgSW, PlacedFacts{}, 16, 10).route == PlacedRoute::Key, "mask defaults to 0");
    expect(subopt_choice(plain, kAlgSW, PlacedFacts{}, 16, 10, 0).route == PlacedRoute::Key, "mask 0 runs");
    expect(subopt_choice(plain, kAlgSW, PlacedFacts{}, 16, 10, 0x7FFFFFFF).route == PlacedRoute::Key, "the largest mask runs");
    expect(subopt_choice(plain, kAlgSW, PlacedFacts{}, 8, 8, 1).key_bits == 3, "8 rows per lane: 3 bits");
    expect(subopt_choice(inputs(lin(2, -1, -3, -3), 2000, 500), kAlgSW, PlacedFacts{0, 0, true}, 64, 32, 1).route == PlacedRoute::Rows, "32 rows per lane: rows");
    // the key's edge, as placed_choice has it: (150 m + 1) << 4 <= 32000 -> m <= 13
    expect(subopt_choice(inputs(lin(13, -1, -3, -3), 150, 500), kAlgSW, PlacedFacts{}, 16, 10, 1).route == PlacedRoute::Key, "match 13: key");
    expect(subopt_choice(inputs(lin(14, -1, -3, -3), 150, 500), kAlgSW, PlacedFacts{}, 16, 10, 1).route == PlacedRoute::Rows, "match 14: rows");
    for (int m : {1, 2, 13, 14, 100, 213})
        for (int K : {8, 10, 16, 32}) {
            const RuleInputs in = inputs(lin(m, -1, -3, -3), 150, 500);
            const PlacedChoice s = subopt_choice(in, kAlgSW, PlacedFacts{}, 64, K, 3), p = placed_choice(in, kAlgSW, PlacedFacts{}, 64, K);
            expect(s.route == p.route && s.key_bits == p.key_bits, "the unbanded placed call's route at match " + std::to_string(m) + " K " + std::to_string(K));
        }

    // ---- 2. what unbanded placed scores refuse, with their texts ----
    auto refused_as_placed = [&](const RuleInputs &in, int alg, const PlacedFacts &f, const char *word) {
        const PlacedChoice c = subopt_choice(in, alg, f, 16, 10, 5);
        expect(c.route == PlacedRoute::Refused && strstr(c.reason, word) != nullptr, std::string("refused with '") + word + "': " + c.reason);
        PlacedFacts unbanded = f;
        unbanded.band_width = 0;
        unbanded.placed_wide = false;
        const PlacedChoice p = placed_choice(in, alg, unbanded, 16, 10);
        expect(p.route == PlacedRoute::Refused && !strcmp(p.reason, c.reason), std::string("placed_choice's own text: ") + c.reason);
    };
    RuleInputs sse = plain;
    sse.sse_policy = true;
    for (bool wide : {false, true}) {
        PlacedFacts f{};
        f.placed_wide = wide;
        refused_as_placed(plain, kAlgNW, f, "Smith-Waterman only");
        refused_as_placed(sse, kAlgSW, f, "traceback_policy");
        f.score_width = 32;
        refused_as_placed(plain, kAlgSW, f, "score_width = 32");
        f.score_width = 0;
        refused_as_placed(inputs(lin(214, -1, -3, -3), 150, 500), kAlgSW, f, "int16");
        expect(subopt_choice(inputs(lin(213, -1, -3, -3), 150, 500), kAlgSW, f, 16, 10, 5).route == PlacedRoute::Rows, "150 x 213: inside int16");
    }
    {
        PlacedFacts wide{};
        wide.placed_wide = true;
        expect(placed_choice(inputs(lin(214, -1, -3, -3), 150, 500), kAlgSW, wide, 16, 10).route == PlacedRoute::Wide, "(placed scores take the int32 sweep there)");
    }
    // ... also first under a band and with a negative mask
    refused_as_placed(plain, kAlgNW, PlacedFacts{64, 0, false, false, true, true}, "Smith-Waterman only");
    expect(strstr(subopt_choice(plain, kAlgNW, PlacedFacts{}, 16, 10, -1).reason, "Smith-Waterman only") != nullptr, "NW before the mask");

    // ---- 3. refusals of its own ----
    for (int mask : {-1, -75, (int)0x80000000}) {
        const PlacedChoice c = subopt_choice(plain, kAlgSW, PlacedFacts{}, 16, 10, mask);
        expect(c.route == PlacedRoute::Refused && !strcmp(c.reason, "suboptimal scores need mask >= 0"), std::string("mask < 0: ") + c.reason);
    }
    const char *band_text = "suboptimal scores are not built for band_width > 0";
    for (bool band_placed : {false, true})
        for (bool usable : {false, true}) {
            const PlacedChoice c = subopt_choice(plain, kAlgSW, PlacedFacts{64, 0, false, false, band_placed, usable}, 16, 10, 5);
            expect(c.route == PlacedRoute::Refused && !strcmp(c.reason, band_text), std::string("band refused: ") + c.reason);
        }
    expect(placed_choice(plain, kAlgSW, PlacedFacts{64, 0, false, false, true, true}, 16, 10).route == PlacedRoute::Chain, "(placed scores do run there)");
    // the strips: more than 1 024 rows unforced, or the long-read plan
    {
        const RuleInputs tall = inputs(lin(2, -1, -3, -3), 1025, 1300);
        expect(placed_choice(tall, kAlgSW, PlacedFacts{}, 64, 24).route == PlacedRoute::Strip, "(1 025 rows: placed scores take the strips)");
        const PlacedChoice c = subopt_choice(tall, kAlgSW, PlacedFacts{}, 64, 24, 5);
        expect(c.route == PlacedRoute::Refused && strstr(c.reason, "register sweep only") != nullptr, std::string("1 025 rows: ") + c.reason);
        expect(subopt_choice(inputs(lin(2, -1, -3, -3), 1024, 1300), kAlgSW, PlacedFacts{}, 64, 16, 5).route == PlacedRoute::Rows, "1 024 rows run (2 049 << 4 is beyond the key)");
        expect(subopt_choice(tall, kAlgSW, PlacedFacts{0, 0, true}, 64, 32, 5).route == PlacedRoute::Rows, "a forced geometry stays on the register sweep");
        PlacedFacts lng{};
        lng.long_plan = true;
        const PlacedChoice d = subopt_choice(plain, kAlgSW, lng, 16, 10, 5);
        expect(d.route == PlacedRoute::Refused && strstr(d.reason, "register sweep only") != nullptr, std::string("no register geometry: ") + d.reason);
    }

    // ---- 4. the ring in the block's LDS: the placed plan's waves halved until tables and rings fit, 0 where one wave's do not ----
    {
        const int limit = 160 * 1024, ring = 1024;
        expect(subopt_block_waves(16864, ring, 4, limit) == 4, "150 x 500 on 16 x 10: four waves, as placed scores");
        expect(subopt_block_waves(40864, ring, 4, limit) == 2, "150 x 3 500: four waves fit without the rings, two with them");
        expect(subopt_block_waves(limit / 4 - ring, ring, 4, limit) == 4 && subopt_block_waves(limit / 4 - ring + 16, ring, 4, limit) == 2, "the edge of four waves");
        expect(subopt_block_waves(limit / 2 - ring, ring, 2, limit) == 2 && subopt_block_waves(limit / 2 - ring + 16, ring, 2, limit) == 1, "the edge of two waves");
        expect(subopt_block_waves(16864, ring, 1, limit) == 1, "never more waves than the placed plan's");
        expect(subopt_block_waves(limit - ring, ring, 1, limit) == 1 && subopt_block_waves(limit - ring + 16, ring, 4, limit) == 0, "one wave's tables and no ring: 0");
        expect(subopt_block_waves(163232, ring, 1, limit) == 0, "150 x 16 200 on 16 x 10: placed scores run, the ring does not fit");
        expect(strstr(kSuboptNoRing, "no room for its column ring") != nullptr, "the refusal's text");
    }

    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("subopt rules ok\n");
    return 0;
}
