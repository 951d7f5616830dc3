// extend_align_rules_check.cpp -- CPU check of extend_align_choice (versalignlib_amd/csrc/cell_rules.h; plain g++, no HIP;
// tests/test_extend_align_rules.py builds and runs it, once more under ASan + UBSan):
//   1. extend_wide = 0: Rows exactly where extend_choice answers Rows, otherwise refused with extend_choice's text -- over a grid
//      of shapes, scorings, score_width 0 / 16 / 32, bands, policy, mode bit, forced geometry, long plan and placed_wide 0 / 1;
//   2. extend_wide = 1: where extend_choice answers Wide, or refuses with its "extend_wide:" text, the call is refused with the
//      text that begins "extension alignments:"; where it answers Rows, Rows; every other refusal keeps its text;
//   3. the pointer scratch per wave: ceil((F + G - 1) / 8) blocks x 64 lanes x K dwords, twice that with affine gaps, on the six
//      full geometries -- with the block count at both sides of a block edge (16 x 10: F = 9 and F = 10 are 3 and 4 blocks) --
//      and nothing without a geometry.
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

}  // namespace

int main() {
    const int shapes[][2] = {{33, 70}, {150, 500}, {1024, 1300}, {1025, 1300}, {1500, 1500}, {10000, 10000}, {5000, 20000}};
    const Scoring scorings[] = {lin(2, -1, -3, -3),          lin(2, -1, -2, -4),           aff(2, -1, -5, -1, -5, -1), aff(2, -1, -6, -2, -4, -1),
                                lin(970, -1, -3, -3),        lin(2, -1, -320, -320),       lin(213, -1, -3, -3),       lin(214, -1, -3, -3),
                                aff(2, -1, -100, -1, -217, -1), aff(2, -1, -100, -1, -218, -1), lin(2, -1, -30000, -30000)};
    long long cells = 0, rows = 0, no_wide = 0, other = 0;
    for (const auto &shape : shapes)
        for (const Scoring &sc : scorings)
            for (int width : {0, 16, 32})
                for (int band : {0, 16})
                    for (bool policy : {false, true})
                        for (int alg : {kAlgSW, kAlgNW})
                            for (int facts_bits = 0; facts_bits < 16; ++facts_bits) {
                                RuleInputs in = inputs(sc, shape[0], shape[1]);
                                in.sse_policy = policy;
                                PlacedFacts f{};
                                f.band_width = band;
                                f.score_width = width;
                                f.forced = facts_bits & 1;
                                f.long_plan = facts_bits & 2;
                                f.placed_wide = facts_bits & 4;
                                f.extend_wide = facts_bits & 8;
                                PlacedFacts narrow = f;
                                narrow.extend_wide = false;
                                const PlacedChoice plain = extend_choice(in, alg, narrow, 16, 10);
                                const PlacedChoice scores = extend_choice(in, alg, f, 16, 10);
                                const ExtendAlignChoice c = extend_align_choice(in, alg, f, 16, 10);
                                const std::string at = "shape " + std::to_string(shape[0]) + " x " + std::to_string(shape[1]) + " width " + std::to_string(width) +
                                                       " band " + std::to_string(band) + " facts " + std::to_string(facts_bits);
                                ++cells;
                                expect(c.route == PlacedRoute::Rows || c.route == PlacedRoute::Refused, at + ": a route other than Rows / Refused");
                                expect((c.route == PlacedRoute::Refused) == (c.reason[0] != 0), at + ": a reason exactly where refused");
                                if (!f.extend_wide) {
                                    expect(c.route == (plain.route == PlacedRoute::Rows ? PlacedRoute::Rows : PlacedRoute::Refused), at + ": key off, route");
                                    expect(std::string(c.reason) == plain.reason, at + ": key off, the extension scores' text");
                                } else if (scores.route == PlacedRoute::Wide || strncmp(scores.reason, "extend_wide:", 12) == 0) {
                                    expect(c.route == PlacedRoute::Refused, at + ": the wide route is refused");
                                    expect(strncmp(c.reason, "extension alignments:", 21) == 0, at + ": the wide route's own text");
                                    expect(std::string(c.reason) == kExtendAlignNoWide, at + ": the wide route's constant");
                                    ++no_wide;
                                } else {
                                    expect(scores.route == plain.route && std::string(scores.reason) == plain.reason, at + ": the key changes nothing here");
                                    expect(c.route == (plain.route == PlacedRoute::Rows ? PlacedRoute::Rows : PlacedRoute::Refused), at + ": key on, route");
                                    expect(std::string(c.reason) == plain.reason, at + ": key on, the extension scores' text");
                                }
                                if (c.route == PlacedRoute::Rows) {
                                    ++rows;
                                    expect(c.blocks8 == (shape[1] + 16 - 1 + 7) / 8, at + ": blocks");
                                    expect(c.wave_ptr_bytes == (long long)c.blocks8 * 64 * 10 * 4 * (sc.affine ? 2 : 1), at + ": bytes per wave");
                                } else {
                                    ++other;
                                    expect(c.blocks8 == 0 && c.wave_ptr_bytes == 0, at + ": a refused call sizes nothing");
                                }
                            }
    expect(rows > 0 && no_wide > 0 && other > no_wide, "the grid reaches every answer");

    // ---- the pointer scratch of a wave ----
    const int full[][2] = {{8, 8}, {16, 10}, {32, 10}, {64, 8}, {64, 16}, {64, 32}};
    for (const auto &g : full)
        for (int F : {1, 7, 8, 9, 10, 100, 500, 1300})
            for (bool affine : {false, true}) {
                const long long blocks = (F + g[0] - 1 + 7) / 8;
                expect(extend_align_wave_ptr_bytes(g[0], g[1], F, affine) == blocks * 64 * g[1] * 4 * (affine ? 2 : 1), "bytes per wave, " + std::to_string(g[0]) + " x " + std::to_string(g[1]));
                PlacedFacts forced{};           // (a forced geometry stays on the register sweep at 2 048 rows too)
                forced.forced = true;
                const ExtendAlignChoice c = extend_align_choice(inputs(affine ? aff(2, -1, -6, -2, -4, -1) : lin(2, -1, -2, -4), g[0] * g[1], F), kAlgSW, forced, g[0], g[1]);
                expect(c.route == PlacedRoute::Rows && c.blocks8 == blocks && c.wave_ptr_bytes == extend_align_wave_ptr_bytes(g[0], g[1], F, affine), "the choice sizes the same");
            }
    // 16 x 10: F = 9 is 24 steps, an exact last block; F = 10 is 25 steps, a block that holds one step
    expect(extend_align_choice(inputs(lin(2, -1, -2, -4), 160, 9), kAlgSW, PlacedFacts{}, 16, 10).blocks8 == 3, "24 steps: 3 blocks");
    expect(extend_align_choice(inputs(lin(2, -1, -2, -4), 160, 10), kAlgSW, PlacedFacts{}, 16, 10).blocks8 == 4, "25 steps: 4 blocks");
    expect(extend_align_wave_ptr_bytes(16, 10, 500, false) == 65ll * 64 * 10 * 4, "150 x 500 on 16 x 10, linear: 166400 bytes per wave of 8 pairs");
    expect(extend_align_wave_ptr_bytes(0, 0, 500, true) == 0, "no geometry: nothing");
    {
        const ExtendAlignChoice c = extend_align_choice(inputs(lin(2, -1, -2, -4), 150, 500), kAlgSW, PlacedFacts{}, 0, 0);
        expect(c.route == PlacedRoute::Rows && c.blocks8 == 0 && c.wave_ptr_bytes == 0, "no geometry: the route alone");
    }

    if (failures) {
        fprintf(stderr, "%d failure(s) over %lld cells\n", failures, cells);
        return 1;
    }
    printf("extend align rules ok (%lld cells: %lld rows, %lld wide refusals, %lld other refusals)\n", cells, rows, no_wide, other);
    return 0;
}
