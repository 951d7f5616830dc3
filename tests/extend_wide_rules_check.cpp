// extend_wide_rules_check.cpp -- CPU check of extend_choice under the extend_wide key and of extend_int32_ok
// (versalignlib_amd/csrc/cell_rules.h; plain g++, no HIP; tests/test_extend_wide_rules.py builds and runs it, once more under
// ASan + UBSan):
//   1. key off: route and reason text equal the rule as it stood before the key (restated below), over a grid of shapes,
//      scorings, score_width 0 / 16 / 32, bands, policy, mode bit, forced geometry, long plan and placed_wide 0 / 1;
//   2. key on: Wide exactly where the key-off rule refuses for score_width = 32, for the int16 range under score_width = 0, or
//      for the register sweep's shapes -- and the key-off answer everywhere else (score_width = 16 out of range, bands, the NW
//      mode bit and policy 1 stay refused, with their texts);
//   3. extend_int32_ok: both sides of its top and its bottom edge, linear and affine, the refusal's own text, and the two
//      sentinel conditions at scores no engine accepts.
#include "cell_rules.h"

#include <stdio.h>
#include <string.h>

#include <string>

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

// The rule before the key: which of its answers a call gets, and the text
enum Before { kNw, kPolicy, kBand, kWidth32, kRange, kSweepOnly, kRows };
const char *const kTexts[] = {
    "extension scores are defined for opt & 0xF == 0 only (the NW variant's free reference start is another matrix)",
    "extension scores are not built for traceback_policy = 1 (SSE/AVX tie-breaks)",
    "extension scores are not built for band_width > 0",
    "extension scores are not built for score_width = 32 (int32 cells)",
    "extension scores run on signed int16 cells: shape x scoring can leave their range",
    "extension scores run on the register sweep only: reads of more than 1024 rows and shapes without a register geometry are refused",
    ""};
Before before(const RuleInputs &in, int alg, const PlacedFacts &f) {
    if (alg != kAlgSW) return kNw;
    if (in.sse_policy) return kPolicy;
    if (f.band_width > 0) return kBand;
    if (f.score_width == 32) return kWidth32;
    if (!(extend_cell_top(in) <= 32000 && extend_cell_bottom(in) >= -32000)) return kRange;
    if (f.long_plan || (!f.forced && in.R > 1024)) return kSweepOnly;
    return kRows;
}

}  // namespace

int main() {
    const int shapes[][2] = {{33, 70}, {150, 500}, {1024, 1300}, {1025, 1300}, {1500, 1500}, {10000, 10000}, {5000, 20000}};
    const Scoring scorings[] = {lin(2, -1, -3, -3),          lin(2, -1, -2, -4),           aff(2, -1, -5, -1, -5, -1), aff(2, -1, -6, -2, -4, -1),
                                lin(970, -1, -3, -3),        lin(2, -1, -320, -320),       lin(213, -1, -3, -3),       lin(214, -1, -3, -3),
                                aff(2, -1, -100, -1, -217, -1), aff(2, -1, -100, -1, -218, -1), lin(2, -1, -30000, -30000)};
    long long cells = 0, wide_cells = 0, wide_refused = 0;
    for (const auto &shape : shapes)
        for (const Scoring &sc : scorings)
            for (int width : {0, 16, 32})
                for (int band : {0, 16})
                    for (bool policy : {false, true})
                        for (int alg : {kAlgSW, kAlgNW})
                            for (int facts_bits = 0; facts_bits < 32; ++facts_bits) {
                                RuleInputs in = inputs(sc, shape[0], shape[1]);
                                in.sse_policy = policy;
                                PlacedFacts f{};
                                f.band_width = band;
                                f.score_width = width;
                                f.forced = facts_bits & 1;
                                f.long_plan = facts_bits & 2;
                                f.placed_wide = facts_bits & 4;
                                f.band_placed = facts_bits & 8;
                                f.chain_usable = facts_bits & 16;
                                const Before was = before(in, alg, f);
                                // ---- 1. key off ----
                                const PlacedChoice off = extend_choice(in, alg, f, 16, 10);
                                expect(off.route == (was == kRows ? PlacedRoute::Rows : PlacedRoute::Refused) && strcmp(off.reason, kTexts[was]) == 0,
                                       std::string("key off decides as before: ") + off.reason + " | " + kTexts[was]);
                                // ---- 2. key on ----
                                f.extend_wide = true;
                                const PlacedChoice on = extend_choice(in, alg, f, 16, 10);
                                const bool opens = was == kWidth32 || (was == kRange && width == 0) || was == kSweepOnly;
                                ++cells;
                                if (!opens) {
                                    expect(on.route == off.route && strcmp(on.reason, off.reason) == 0, std::string("key on, elsewhere: as with the key off: ") + on.reason);
                                } else if (extend_int32_ok(in)) {
                                    ++wide_cells;
                                    expect(on.route == PlacedRoute::Wide && on.reason[0] == 0, std::string("key on: Wide, no reason: ") + on.reason);
                                } else {
                                    ++wide_refused;
                                    expect(on.route == PlacedRoute::Refused && strncmp(on.reason, "extend_wide:", 12) == 0, std::string("key on, beyond int32: ") + on.reason);
                                }
                            }
    expect(cells > 10000 && wide_cells > 500 && wide_refused > 50, "the grid reaches every answer");

    // the three places by name, and what stays refused
    {
        PlacedFacts f{};
        f.extend_wide = true;
        const RuleInputs plain = inputs(lin(2, -1, -3, -3), 150, 500);
        expect(extend_choice(plain, kAlgSW, f, 16, 10).route == PlacedRoute::Rows, "in range, short read, key on: the register sweep keeps the call");
        f.score_width = 32;
        expect(extend_choice(plain, kAlgSW, f, 16, 10).route == PlacedRoute::Wide, "score_width = 32");
        f.score_width = 0;
        expect(extend_choice(inputs(lin(970, -1, -3, -3), 33, 70), kAlgSW, f, 16, 10).route == PlacedRoute::Wide, "match 970 at 33 x 70");
        expect(extend_choice(inputs(lin(2, -1, -320, -320), 33, 70), kAlgSW, f, 16, 10).route == PlacedRoute::Wide, "gaps of -320 at 33 x 70");
        expect(extend_choice(inputs(lin(2, -1, -3, -3), 1025, 1300), kAlgSW, f, 16, 10).route == PlacedRoute::Wide, "1 025 rows");
        expect(extend_choice(inputs(lin(2, -1, -3, -3), 1024, 1300), kAlgSW, f, 16, 10).route == PlacedRoute::Rows, "1 024 rows: the register sweep");
        PlacedFacts lng = f;
        lng.long_plan = true;
        expect(extend_choice(plain, kAlgSW, lng, 16, 10).route == PlacedRoute::Wide, "no register geometry");
        PlacedFacts forced = f;
        forced.forced = true;
        expect(extend_choice(inputs(lin(2, -1, -3, -3), 1025, 1300), kAlgSW, forced, 64, 32).route == PlacedRoute::Rows, "a forced geometry stays on the register sweep");
        f.score_width = 16;
        const PlacedChoice c16 = extend_choice(inputs(lin(970, -1, -3, -3), 33, 70), kAlgSW, f, 16, 10);
        expect(c16.route == PlacedRoute::Refused && strstr(c16.reason, "signed int16 cells"), "score_width = 16 out of range stays refused");
        f.score_width = 32;
        expect(strstr(extend_choice(plain, kAlgNW, f, 16, 10).reason, "opt & 0xF == 0 only") != nullptr, "the NW mode bit stays refused");
        RuleInputs sse = plain;
        sse.sse_policy = true;
        expect(strstr(extend_choice(sse, kAlgSW, f, 16, 10).reason, "traceback_policy = 1") != nullptr, "policy 1 stays refused");
        f.band_width = 64;
        f.band_placed = f.chain_usable = true;
        expect(strstr(extend_choice(plain, kAlgSW, f, 16, 10).reason, "not built for band_width > 0") != nullptr, "a band stays refused");
        // placed_wide opens nothing here
        PlacedFacts pw{};
        pw.placed_wide = true;
        pw.score_width = 32;
        expect(extend_choice(plain, kAlgSW, pw, 16, 10).route == PlacedRoute::Refused, "placed_wide alone opens nothing for extension calls");
    }

    // ---- 3. extend_int32_ok, both sides of each edge (2^28 = 268 435 456) ----
    expect(kExtendWideCellBound == 268435456ll && kExtendWideLoses == -536870912, "the bound and the sentinel");
    // top: min(R, F) x max(match, mismatch, 0): 16384 x 16384 = 2^28 | 16384 x 16385
    expect(extend_cell_top(inputs(lin(16384, -1, 0, 0), 16384, 16384)) == kExtendWideCellBound, "16384 x 16384 is the bound");
    expect(extend_int32_ok(inputs(lin(16384, 0, 0, 0), 16384, 16384)) && !extend_int32_ok(inputs(lin(16385, 0, 0, 0), 16384, 16384)), "top: match 16384 | 16385");
    expect(extend_int32_ok(inputs(lin(1, 16384, 0, 0), 16384, 16384)) && !extend_int32_ok(inputs(lin(1, 16385, 0, 0), 16384, 16384)), "top: a positive mismatch counts");
    expect(extend_int32_ok(inputs(lin(26843, 0, 0, 0), 10000, 20000)) && !extend_int32_ok(inputs(lin(26844, 0, 0, 0), 10000, 20000)), "top: the shorter side, 10000 x 26843 | 26844");
    // bottom, linear: R gap_ref + F gap_read + the largest addend: 8192 x -16384 x 2 = -2^28 exactly with a zero addend ...
    expect(extend_cell_bottom(inputs(lin(0, 0, -16384, -16384), 8192, 8192)) == -kExtendWideCellBound - 16384, "the addend is the gap itself");
    expect(extend_int32_ok(inputs(lin(2, -1, -13421, -13421), 10000, 10000)) && !extend_int32_ok(inputs(lin(2, -1, -13422, -13422), 10000, 10000)),
           "bottom: 20000 steps at -13421 | -13422: -268 433 421 | -268 453 422");
    expect(extend_int32_ok(inputs(lin(2, -15456, -13421, -13421), 10000, 10000)) && !extend_int32_ok(inputs(lin(2, -15457, -13421, -13421), 10000, 10000)),
           "bottom: the addend is the mismatch where it is the largest: -268 435 456 | -268 435 457");
    // bottom, affine: every step at the worse of open and extend
    expect(extend_int32_ok(inputs(aff(2, -1, -13421, -1, -13421, -1), 10000, 10000)) && !extend_int32_ok(inputs(aff(2, -1, -13422, -1, -13421, -1), 10000, 10000)),
           "bottom, affine: the openings price the steps");
    expect(extend_int32_ok(inputs(lin(2, -1, -30000, -30000), 33, 70)) && !extend_int32_ok(inputs(lin(2, -1, -30000, -30000), 5000, 5000)), "gaps of -30000: 33 x 70 | 5000 x 5000");
    {
        PlacedFacts f{};
        f.extend_wide = true;
        const PlacedChoice c = extend_choice(inputs(lin(2, -1, -30000, -30000), 5000, 5000), kAlgSW, f, 16, 10);
        expect(c.route == PlacedRoute::Refused && strncmp(c.reason, "extend_wide:", 12) == 0, std::string("the refusal's own text: ") + c.reason);
        f.extend_wide = false;
        expect(strstr(extend_choice(inputs(lin(2, -1, -30000, -30000), 5000, 5000), kAlgSW, f, 16, 10).reason, "signed int16 cells") != nullptr, "... and the key-off text");
    }
    // the sentinel's two conditions hold for every int16 scoring; scores no engine accepts reach them
    expect(extend_int32_ok(inputs(lin(32767, 32767, -32768, -32768), 1, 1)), "int16 scores: the sentinel plus an addend stays below the bound");
    expect(!extend_int32_ok(inputs(lin(kExtendWideCellBound, 0, 0, 0), 1, 1)), "sentinel + match 2^28 reaches -2^28: refused (the top is the bound itself)");
    expect(extend_int32_ok(inputs(lin(2, 0, -8000, -8000), 16383, 16384)) && !extend_int32_ok(inputs(lin(2, 0, -49153, 0), 0, 32767)),
           "the drift: 2^29 + 32767 x 49153 leaves int32 (the cells themselves stay above -2^28 there: R = 0)");

    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("extend wide rules ok\n");
    return 0;
}
