// placed_wide_rules_check.cpp -- CPU check of placed_choice and span_choice under placed_wide (versalignlib_amd/csrc/cell_rules.h;
// plain g++, no HIP; tests/test_placed_wide_rules.py builds it with -fsanitize=address,undefined and runs it):
//   1. the key off: over a grid of shapes, scorings, score_width, bands and policies the route and the reason are those of a
//      PlacedFacts that does not know the member -- nothing changes by default;
//   2. the key on: Wide exactly where the two int16 refusals applied, found through the edge of int16_range_ok (150 x 500:
//      match 213 against 214); score_width = 16 beyond the edge keeps the old refusal; in-range calls keep Key / Rows / Strip;
//   3. the int32_refused edge, one step either side of (R + F + 2) * worst = 2^28: Wide against the `placed_wide:` refusal;
//   4. the NW variant, traceback_policy = 1 and a band without band_placed keep their refusals; a band with band_placed is Chain.
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

bool same(const PlacedChoice &a, const PlacedChoice &b) { return a.route == b.route && a.key_bits == b.key_bits && !strcmp(a.reason, b.reason); }

const char *const kWidth32 = "placed scores are not built for score_width = 32 (int32 cells)";
const char *const kRange16 = "placed scores run on int16 cells: shape x scoring can leave their range";
const char *const kBand = "placed scores are not built for band_width > 0";
const char *const kWideRange = "placed_wide: shape x scoring can leave the int32 range of the DP cells";

// today's rule, restated: what a call without the key is (the cascade of placed_choice before this key existed)
PlacedChoice todays_rule(const RuleInputs &in, int alg, PlacedFacts f, int G, int K) {
    f.placed_wide = false;
    return placed_choice(in, alg, f, G, K);
}

}  // namespace

int main() {
    // ---- 0. the new member is the last one and defaults to off: the positional brace initialisers mean what they meant ----
    expect(!PlacedFacts{}.placed_wide && !PlacedFacts{64, 0, false, false}.placed_wide && !PlacedFacts{0, 32, false, false, true, true}.placed_wide,
           "placed_wide defaults to false");
    expect((PlacedFacts{0, 32, false, false, false, false, true}.placed_wide), "placed_wide is the seventh member");
    expect((int)PlacedRoute::Wide == 5 && (int)PlacedRoute::Chain == 4 && (int)PlacedRoute::Refused == 0, "Wide is appended to PlacedRoute");
    expect(!strcmp(ran_placed_name(PlacedRoute::Wide), "wide") && !strcmp(ran_placed_name(PlacedRoute::Chain), "chain") &&
               !strcmp(ran_placed_name(PlacedRoute::Strip), "strip") && !strcmp(ran_placed_name(PlacedRoute::Refused), "none"),
           "describe()'s names");

    // ---- 1. key off: nothing changes; never Wide, and the two refusals keep their texts ----
    int refused_32 = 0, refused_range = 0;
    for (int R : {12, 150, 1024, 1025, 5000, 10000})
        for (int F : {130, 500, 10000})
            for (int match : {1, 2, 5, 14, 100, 213, 214, 600})
                for (int sw : {0, 16, 32})
                    for (int band : {0, 64})
                        for (int flags = 0; flags < 16; ++flags)
                            for (int alg : {kAlgSW, kAlgNW}) {
                                RuleInputs in = inputs(flags & 4 ? aff(match, -1, -5, -1, -5, -1) : lin(match, -1, -3, -3), R, F);
                                in.sse_policy = (flags & 1) != 0;
                                const PlacedFacts off{band, sw, (flags & 2) != 0, R > 2048, (flags & 8) != 0, true, false};
                                const PlacedFacts plain{band, sw, (flags & 2) != 0, R > 2048, (flags & 8) != 0, true};       // six members: the struct before the key
                                for (int K : {8, 24}) {
                                    const PlacedChoice c = placed_choice(in, alg, off, 64, K);
                                    expect(same(c, placed_choice(in, alg, plain, 64, K)), "key off: the choice of a PlacedFacts without the member");
                                    expect(same(span_choice(in, alg, off, 64, K), span_choice(in, alg, plain, 64, K)), "key off: span_choice likewise");
                                    expect(c.route != PlacedRoute::Wide && span_choice(in, alg, off, 64, K).route != PlacedRoute::Wide, "key off: never Wide");
                                    if (c.route == PlacedRoute::Refused) expect(strncmp(c.reason, "placed_wide:", 12) != 0, "key off: never the key's refusal");
                                    if (!strcmp(c.reason, kWidth32)) ++refused_32;
                                    if (!strcmp(c.reason, kRange16)) ++refused_range;
                                    // ---- 2a. key on, over the same grid: Wide exactly where one of the two refusals applied and score_width is not 16
                                    PlacedFacts on = off;
                                    on.placed_wide = true;
                                    const PlacedChoice w = placed_choice(in, alg, on, 64, K);
                                    const bool was_cells = !strcmp(c.reason, kWidth32) || !strcmp(c.reason, kRange16);
                                    if (was_cells && sw != 16) {
                                        expect(!int32_refused(in), "the grid stays inside int32");
                                        expect(w.route == PlacedRoute::Wide && w.reason[0] == 0 && w.key_bits == 0, std::string("key on: Wide where today refuses for the cells: ") + c.reason);
                                        expect(band == 0 && alg == kAlgSW && !in.sse_policy, "... which is unbanded Smith-Waterman with the default tie-breaks");
                                    } else {
                                        expect(same(w, c), std::string("key on: every other call as with the key off: ") + c.reason + " / " + w.reason);
                                    }
                                    // span_choice follows placed_choice without a band, and refuses a band by name where the rest would run
                                    const PlacedChoice s = span_choice(in, alg, on, 64, K);
                                    PlacedFacts unbanded = on;
                                    unbanded.band_width = 0;
                                    const PlacedChoice u = placed_choice(in, alg, unbanded, 64, K);
                                    if (band == 0) expect(same(s, w), "span_choice is placed_choice without a band");
                                    else if (u.route != PlacedRoute::Refused) expect(s.route == PlacedRoute::Refused && !strcmp(s.reason, "spanned scores are not built for band_width > 0"), "spanned scores under a band");
                                    else expect(same(s, u), "spanned scores: the unbanded refusal first");
                                }
                            }
    expect(refused_32 > 0 && refused_range > 0, "the grid meets both refusals");

    // ---- 2b. the edge of int16_range_ok at 150 x 500: min(R, F) * match + 1 > 32000 first at match 214 ----
    {
        int last_ok = -1, changes = 0;
        bool prev = true;
        for (int match = 1; match <= 400; ++match) {
            const RuleInputs in = inputs(lin(match, -1, -3, -3), 150, 500);
            const bool ok = int16_range_ok(in, kAlgSW, true, false, 0);
            if (ok != prev) {
                ++changes;
                last_ok = match - 1;
            }
            prev = ok;
            PlacedFacts on{};
            on.placed_wide = true;
            const PlacedChoice c = placed_choice(in, kAlgSW, on, 64, 8);
            expect((c.route == PlacedRoute::Wide) == !ok, "score_width 0: Wide exactly beyond the int16 edge (match " + std::to_string(match) + ")");
            if (ok) expect(c.route == PlacedRoute::Key || c.route == PlacedRoute::Rows, "inside the edge: the register sweep");
            expect(same(c, span_choice(in, kAlgSW, on, 64, 8)), "span_choice follows");
            on.score_width = 16;
            const PlacedChoice c16 = placed_choice(in, kAlgSW, on, 64, 8);
            if (ok) expect(c16.route == PlacedRoute::Key || c16.route == PlacedRoute::Rows, "score_width 16 inside the edge runs");
            else expect(c16.route == PlacedRoute::Refused && !strcmp(c16.reason, kRange16), "score_width 16 beyond the edge: int16 or refuse, today's text");
            on.score_width = 32;
            expect(placed_choice(in, kAlgSW, on, 64, 8).route == PlacedRoute::Wide, "score_width 32 with the key: Wide on either side");
            on.placed_wide = false;
            const PlacedChoice off32 = placed_choice(in, kAlgSW, on, 64, 8);
            expect(off32.route == PlacedRoute::Refused && !strcmp(off32.reason, kWidth32), "score_width 32 without the key: today's text");
        }
        expect(changes == 1 && last_ok == 213, "150 x 500: match 213 is the last inside int16, found " + std::to_string(last_ok));
    }
    // ... and the shapes the key was asked for
    {
        PlacedFacts on{};
        on.placed_wide = true;
        PlacedFacts on_long = on;
        on_long.long_plan = true;
        expect(placed_choice(inputs(lin(2, -1, -3, -3), 20000, 20000), kAlgSW, on_long, 64, 8).route == PlacedRoute::Wide, "20 kbp x 20 kbp at match 2");
        expect(placed_choice(inputs(aff(5, -4, -8, -2, -8, -2), 10000, 10000), kAlgSW, on_long, 64, 8).route == PlacedRoute::Wide, "10 kbp x 10 kbp at match 5");
        expect(placed_choice(inputs(lin(300, -4, -6, -6), 150, 500), kAlgSW, on, 64, 8).route == PlacedRoute::Wide, "150 x 500 at match 300");
        // in-range calls keep their routes and their key bits
        expect(placed_choice(inputs(lin(2, -1, -3, -3), 150, 500), kAlgSW, on, 16, 10).route == PlacedRoute::Key, "150 x 500 at match 2: the key");
        expect(placed_choice(inputs(lin(2, -1, -3, -3), 150, 500), kAlgSW, on, 16, 10).key_bits == placed_key_bits(10), "... with its bits");
        expect(placed_choice(inputs(lin(100, -1, -3, -3), 150, 500), kAlgSW, on, 16, 10).route == PlacedRoute::Rows, "150 x 500 at match 100: per row");
        expect(placed_choice(inputs(lin(2, -1, -3, -3), 1025, 130), kAlgSW, on, 64, 24).route == PlacedRoute::Strip, "1025 x 130: the strips");
        expect(placed_choice(inputs(lin(2, -1, -3, -3), 5000, 5000), kAlgSW, on_long, 64, 24).route == PlacedRoute::Strip, "5 kbp x 5 kbp at match 2: the strips");
    }

    // ---- 3. the int32_refused edge: (R + F + 2) * worst = 2^28, one step either side ----
    for (int side : {4100, 9000}) {
        const long long last = ((1ll << 28) - 1) / (2 * side + 2);         // the largest |score| with (R + F + 2) * |score| < 2^28
        expect(last <= 32767 && (2 * side + 2) * last < (1ll << 28) && (2 * side + 2) * (last + 1) >= (1ll << 28), "the edge is inside short scores");
        for (bool by_match : {true, false}) {
            // worst = match, or worst = |gap| with a small match that is out of int16 by score_width = 32 only
            const RuleInputs in_ok = inputs(by_match ? lin((int)last, -1, -3, -3) : lin(2, -1, -(int)last, -3), side, side);
            const RuleInputs in_bad = inputs(by_match ? lin((int)last + 1, -1, -3, -3) : lin(2, -1, -(int)last - 1, -3), side, side);
            PlacedFacts on{0, 32, false, true};
            on.placed_wide = true;
            expect(!int32_refused(in_ok) && int32_refused(in_bad), "int32_refused flips here");
            const PlacedChoice ok = placed_choice(in_ok, kAlgSW, on, 64, 8), bad = placed_choice(in_bad, kAlgSW, on, 64, 8);
            expect(ok.route == PlacedRoute::Wide, "the last score inside int32 is Wide");
            expect(bad.route == PlacedRoute::Refused && !strcmp(bad.reason, kWideRange) && !strncmp(bad.reason, "placed_wide:", 12), std::string("the next one is refused by name: ") + bad.reason);
            expect(same(span_choice(in_bad, kAlgSW, on, 64, 8), bad) && same(span_choice(in_ok, kAlgSW, on, 64, 8), ok), "span_choice follows");
            on.placed_wide = false;
            expect(!strcmp(placed_choice(in_bad, kAlgSW, on, 64, 8).reason, kWidth32), "key off: today's text, not the key's");
        }
    }

    // ---- 4. what the key does not touch ----
    for (const RuleInputs &base : {inputs(lin(300, -4, -6, -6), 150, 500), inputs(aff(5, -4, -8, -2, -8, -2), 10000, 10000), inputs(lin(2, -1, -3, -3), 150, 500)})
        for (int sw : {0, 32}) {
            PlacedFacts on{0, sw, false, base.R > 2048};
            on.placed_wide = true;
            const PlacedChoice nw = placed_choice(base, kAlgNW, on, 64, 8);
            expect(nw.route == PlacedRoute::Refused && same(nw, todays_rule(base, kAlgNW, on, 64, 8)) && strstr(nw.reason, "Smith-Waterman only") != nullptr, "the NW variant is refused as ever");
            RuleInputs sse = base;
            sse.sse_policy = true;
            const PlacedChoice pol = placed_choice(sse, kAlgSW, on, 64, 8);
            expect(pol.route == PlacedRoute::Refused && same(pol, todays_rule(sse, kAlgSW, on, 64, 8)) && strstr(pol.reason, "traceback_policy = 1") != nullptr, "traceback_policy = 1 is refused as ever");
            PlacedFacts banded = on;
            banded.band_width = 64;
            const PlacedChoice b = placed_choice(base, kAlgSW, banded, 64, 8);
            expect(b.route == PlacedRoute::Refused && !strcmp(b.reason, kBand), "a band without band_placed is refused as ever");
            banded.band_placed = true;
            banded.chain_usable = true;
            const PlacedChoice ch = placed_choice(base, kAlgSW, banded, 64, 8);
            expect(ch.route == PlacedRoute::Chain && ch.key_bits == kBandPlacedKeyBits, "a band with band_placed is the chain: the key is not read under a band");
            banded.chain_usable = false;
            expect(same(placed_choice(base, kAlgSW, banded, 64, 8), todays_rule(base, kAlgSW, banded, 64, 8)), "... and an unusable plan keeps its refusal");
        }

    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("placed wide rules ok\n");
    return 0;
}
