// extend_band_rules_check.cpp -- CPU check of the extend_band key's rule and plan (versalignlib_amd/csrc/cell_rules.h and
// extend_band_plan.h; plain g++, no HIP; tests/test_extend_band_rules.py builds and runs it, once more under ASan + UBSan):
//   1. extend_choice: key off, or no band -- route and reason as with the key absent, whatever extend_wide says; key on under a
//      band -- the mode bit's and the policy's texts first, then score_width = 16, then the int32 bound, each with its own text,
//      otherwise Band, whatever the read length, score_width 0 / 32 and extend_wide say;
//   2. extend_align_choice: under a band with the key on the text starts "extension alignments: not built under a band" (after
//      the mode bit and the policy), with the key off today's text; without a band the key changes nothing;
//   3. extend_band_int32_ok at its edges: the diagonal steps count, the top and the sentinel's conditions are extend_int32_ok's;
//   4. the window functions against a direct enumeration of the present cells -- a block's window is the union of its rows'
//      per-cell windows |i - j| <= w -- for small and three-strip shapes, w = 0 and strips with an empty window included: a
//      strip's first and last column and step, emptiness, the borders, the unreached rule, the row above a strip, and that
//      every present cell has a present predecessor.
#include "cell_rules.h"
#include "extend_band_plan.h"

#include <stdio.h>
#include <stdlib.h>
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

const char *const kNwText = "extension scores are defined for opt & 0xF == 0 only (the NW variant's free reference start is another matrix)";
const char *const kPolicyText = "extension scores are not built for traceback_policy = 1 (SSE/AVX tie-breaks)";
const char *const kBandText = "extension scores are not built for band_width > 0";
const char *const kAlignBandStart = "extension alignments: not built under a band";

// the band restated: cell (i, j), i >= -1, j >= -1, is present iff a row of its block lies within w diagonals of the column
bool present_direct(int i, int j, int w) {
    if (i < 0) return abs(i - j) <= w;
    for (int r = i / 8 * 8; r < i / 8 * 8 + 8; ++r)
        if (abs(r - j) <= w) return true;
    return false;
}

}  // namespace

int main() {
    // ---- 1. and 2. the two choices over a grid ----
    const int shapes[][2] = {{33, 70}, {150, 500}, {1024, 1300}, {1025, 1300}, {10000, 10000}, {5000, 20000}};
    const Scoring scorings[] = {lin(2, -1, -3, -3), lin(2, -1, -2, -4), aff(2, -1, -5, -1, -5, -1), aff(2, -1, -6, -2, -4, -1),
                                lin(970, -1, -3, -3), lin(2, -1, -320, -320), lin(2, -1, -30000, -30000), lin(30000, -1, -3, -3)};
    long long cells = 0, band_cells = 0, band_range = 0, band_16 = 0;
    for (const auto &shape : shapes)
        for (const Scoring &sc : scorings)
            for (int width : {0, 16, 32})
                for (int band : {0, 1, 16, 1000})
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
                                f.extend_wide = facts_bits & 4;
                                f.band_placed = f.chain_usable = facts_bits & 8;
                                const PlacedChoice off = extend_choice(in, alg, f, 16, 10);
                                const ExtendAlignChoice align_off = extend_align_choice(in, alg, f, 16, 10);
                                f.extend_band = true;
                                const PlacedChoice on = extend_choice(in, alg, f, 16, 10);
                                const ExtendAlignChoice align_on = extend_align_choice(in, alg, f, 16, 10);
                                ++cells;
                                expect(off.route != kPlacedRouteBand, "key off: never Band");
                                if (band == 0) {
                                    expect(on.route == off.route && strcmp(on.reason, off.reason) == 0, std::string("no band: the key is not read: ") + on.reason);
                                    expect(align_on.route == align_off.route && strcmp(align_on.reason, align_off.reason) == 0 && align_on.wave_ptr_bytes == align_off.wave_ptr_bytes,
                                           std::string("no band: alignments do not read the key: ") + align_on.reason);
                                    continue;
                                }
                                // key off under a band: refused, today's texts
                                const char *first = alg != kAlgSW ? kNwText : (policy ? kPolicyText : kBandText);
                                expect(off.route == PlacedRoute::Refused && strcmp(off.reason, first) == 0, std::string("key off under a band: ") + off.reason);
                                expect(align_off.route == PlacedRoute::Refused && strcmp(align_off.reason, first) == 0, std::string("alignments, key off under a band: ") + align_off.reason);
                                // key on under a band
                                if (alg != kAlgSW || policy) {
                                    expect(on.route == PlacedRoute::Refused && strcmp(on.reason, first) == 0, std::string("key on: the mode bit and the policy keep their texts: ") + on.reason);
                                    expect(align_on.route == PlacedRoute::Refused && strcmp(align_on.reason, first) == 0, std::string("alignments, key on: mode bit / policy: ") + align_on.reason);
                                    continue;
                                }
                                expect(align_on.route == PlacedRoute::Refused && strncmp(align_on.reason, kAlignBandStart, strlen(kAlignBandStart)) == 0 && align_on.wave_ptr_bytes == 0,
                                       std::string("alignments, key on under a band: ") + align_on.reason);
                                if (width == 16) {
                                    ++band_16;
                                    expect(on.route == PlacedRoute::Refused && on.reason == kExtendBandNoInt16 && strncmp(on.reason, "extend_band:", 12) == 0, std::string("score_width = 16: ") + on.reason);
                                } else if (!extend_band_int32_ok(in)) {
                                    ++band_range;
                                    expect(on.route == PlacedRoute::Refused && on.reason == kExtendBandRange && strncmp(on.reason, "extend_band:", 12) == 0, std::string("beyond the band's int32 bound: ") + on.reason);
                                } else {
                                    ++band_cells;
                                    expect(on.route == kPlacedRouteBand && on.reason[0] == 0, std::string("key on under a band: Band: ") + on.reason);
                                }
                            }
    expect(cells > 10000 && band_cells > 1000 && band_range > 50 && band_16 > 500, "the grid reaches every answer");
    expect(strcmp(kExtendBandNoInt16, kExtendBandRange) != 0 && strcmp(ran_placed_name(kPlacedRouteBand), "band") == 0 && strcmp(ran_placed_name(PlacedRoute::Wide), "wide") == 0,
           "two texts; describe's name of the route");
    {
        // by name: a short read the register sweep would serve runs banded on the strips; the default facts have the key off
        PlacedFacts f{};
        expect(!f.extend_band, "the key is off by default");
        PlacedFacts six{16, 0, false, false, false, false};         // an aggregate initialiser from before the keys still compiles
        expect(six.band_width == 16 && !six.extend_wide && !six.extend_band, "trailing members default to false");
        f.band_width = 9;
        f.extend_band = true;
        expect(extend_choice(inputs(lin(2, -1, -3, -3), 150, 500), kAlgSW, f, 16, 10).route == kPlacedRouteBand, "150 x 500 under a band");
        f.score_width = 32;
        expect(extend_choice(inputs(lin(2, -1, -3, -3), 10000, 10000), kAlgSW, f, 0, 0).route == kPlacedRouteBand, "10 kbp under a band, score_width = 32");
    }

    // ---- 3. extend_band_int32_ok at its edges (2^28 = 268 435 456) ----
    {
        const RuleInputs a = inputs(lin(2, -7, -11, -13), 300, 200), b = inputs(aff(5, -4, -8, -2, -9, -3), 200, 300);
        expect(extend_band_cell_bottom(a) == extend_cell_bottom(a) - 7 * 200 && extend_band_cell_bottom(a) == -13ll * 300 - 11 * 200 - 7 * 200 - 13, "bottom, linear: the diagonal steps are added");
        expect(extend_band_cell_bottom(b) == extend_cell_bottom(b) - 4 * 200 && extend_band_cell_bottom(b) == -9ll * 200 - 8 * 300 - 4 * 200 - 9, "bottom, affine");
        expect(extend_band_cell_bottom(inputs(lin(2, 1, -3, -3), 50, 60)) == extend_cell_bottom(inputs(lin(2, 1, -3, -3), 50, 60)), "no negative substitution score: the unbanded bottom");
    }
    // 20000 gap steps and 10000 diagonal steps: 20001 x 13420 + 10000 = 268 423 420 | 20001 x 13421 + 10000 = 268 443 421
    expect(extend_band_int32_ok(inputs(lin(2, -1, -13420, -13420), 10000, 10000)) && !extend_band_int32_ok(inputs(lin(2, -1, -13421, -13421), 10000, 10000)), "bottom: gaps of -13420 | -13421");
    expect(extend_int32_ok(inputs(lin(2, -1, -13421, -13421), 10000, 10000)) && extend_band_int32_ok(inputs(lin(2, 0, -13421, -13421), 10000, 10000)),
           "... which the unbanded bound takes, and the band's without a negative mismatch");
    // 268 400 000 + 10000 |mismatch| + 13420: mismatch -2 -> 268 433 420 | -3 -> 268 443 420
    expect(extend_band_int32_ok(inputs(lin(2, -2, -13420, -13420), 10000, 10000)) && !extend_band_int32_ok(inputs(lin(2, -3, -13420, -13420), 10000, 10000)), "bottom: mismatch -2 | -3");
    // the shorter side prices the diagonal steps: 5000 x 20000: 25000 x 10000 + 5000 x 3686 + 10000 = 268 440 000 | 3685: 268 435 000
    expect(extend_band_int32_ok(inputs(lin(2, -3685, -10000, -10000), 5000, 20000)) && !extend_band_int32_ok(inputs(lin(2, -3686, -10000, -10000), 5000, 20000)), "bottom: min(R, F) diagonal steps");
    expect(extend_band_int32_ok(inputs(aff(2, 0, -13421, -1, -13421, -1), 10000, 10000)) && !extend_band_int32_ok(inputs(aff(2, 0, -13422, -1, -13421, -1), 10000, 10000)), "bottom, affine: the openings price the steps");
    expect(extend_band_int32_ok(inputs(lin(16384, 0, 0, 0), 16384, 16384)) && !extend_band_int32_ok(inputs(lin(16385, 0, 0, 0), 16384, 16384)), "top: as extend_int32_ok");
    expect(extend_band_int32_ok(inputs(lin(32767, 32767, -32768, -32768), 1, 1)) && !extend_band_int32_ok(inputs(lin(kExtendWideCellBound, 0, 0, 0), 1, 1)), "the sentinel plus an addend");
    expect(extend_band_int32_ok(inputs(lin(2, 0, -8000, -8000), 16383, 16384)) && !extend_band_int32_ok(inputs(lin(2, 0, -49153, 0), 0, 32767)), "the drift");

    // ---- 4. the window functions against a direct enumeration ----
    expect(kExtendBandBlockRows == 8 && VALIGN_HIP_EXTEND_BAND_BLOCK_ROWS == 8 && kExtendBandStripRows == 512 && kExtendBandColAlign == 64, "the constants");
    expect(VALIGN_HIP_EXTEND_UNREACHED == -2147483647 - 1, "UNREACHED is INT32_MIN");
    expect(extend_band_half(1, 33, 70) == 0 && extend_band_half(2, 33, 70) == 1 && extend_band_half(9, 33, 70) == 4 && extend_band_half(139, 33, 70) == 69 &&
               extend_band_half(140, 33, 70) == 70 && extend_band_half(400, 33, 70) == 70 && extend_band_half(0x7FFFFFFF, 70, 33) == 70,
           "w = band_width / 2, capped at the unbanded limit max(R, F)");
    long long checked = 0, empties = 0, unreached_seen = 0;
    for (int w : {0, 1, 2, 3, 4, 7, 8, 9, 20, 63, 64, 65, 100, 300, 600, 1200}) {
        // cells, borders, predecessors: a small matrix
        for (int i = -1; i < 40; ++i)
            for (int j = -1; j < 60; ++j) {
                const bool p = present_direct(i, j, w);
                expect(extend_band_present(i, j, w) == p, "present: cell " + std::to_string(i) + "," + std::to_string(j) + " w " + std::to_string(w));
                if (j == -1) expect(extend_band_border_col_present(i, w) == p, "the border column, row " + std::to_string(i));
                if (i == -1) expect(extend_band_border_row_present(j, w) == p, "the border row, column " + std::to_string(j));
                if (i >= 0) expect(p == (extend_band_lo(i, w) <= j && j <= extend_band_hi(i, w)), "a block's [lo, hi]");
                if (p && !(i == -1 && j == -1)) {
                    const bool pred = (i >= 0 && j >= 0 && present_direct(i - 1, j - 1, w)) || (i >= 0 && present_direct(i - 1, j, w)) || (j >= 0 && present_direct(i, j - 1, w));
                    expect(pred, "a present cell has a present predecessor: " + std::to_string(i) + "," + std::to_string(j) + " w " + std::to_string(w));
                }
                ++checked;
            }
        expect(extend_band_present(-1, -1, w) && extend_band_border_col_present(-1, w), "the origin is present");
        // the unreached rule: row Rp - 1 has no present candidate -1 <= j < Fp
        for (int Rp = 0; Rp < 45; ++Rp)
            for (int Fp = 0; Fp < 45; ++Fp) {
                bool any = false;
                for (int j = -1; j < Fp && Rp > 0; ++j) any = any || present_direct(Rp - 1, j, w);
                expect(extend_band_unreached(Rp, Fp, w) == (Rp > 0 && !any), "unreached: Rp " + std::to_string(Rp) + " Fp " + std::to_string(Fp) + " w " + std::to_string(w));
                unreached_seen += Rp > 0 && !any;
            }
        // a strip's window: the columns 0 <= j < F its 512 rows hold a present cell in
        for (int F : {0, 1, 63, 64, 65, 129, 511, 512, 600, 1100, 1700})
            for (int strip = 0; strip < 3; ++strip) {
                int first = -1, last = -1;
                for (int j = 0; j < F; ++j) {
                    bool any = false;
                    for (int b = 0; b < 64 && !any; ++b) any = present_direct(strip * 512 + 8 * b, j, w);
                    if (any) {
                        if (first < 0) first = j;
                        last = j;
                    }
                }
                const ExtendBandStrip s = extend_band_strip(strip, F, w);
                const std::string at = "strip " + std::to_string(strip) + " F " + std::to_string(F) + " w " + std::to_string(w);
                expect(s.empty == (first < 0), "a strip's window is empty: " + at);
                empties += s.empty;
                if (first >= 0) {
                    expect(s.col_first == first && s.col_end == last + 1, "a strip's first and last column: " + at);
                    expect(s.t_begin % 64 == 0 && s.t_begin <= first && first < s.t_begin + 64, "the first step: the 64-column block of the first column: " + at);
                    expect(s.t_end == last + 64, "the last step: lane 63 sweeps the last column: " + at);
                    for (int j = first; j <= last; ++j) {       // (a window has no hole)
                        bool any = false;
                        for (int b = 0; b < 64 && !any; ++b) any = present_direct(strip * 512 + 8 * b, j, w);
                        expect(any, "a window without a hole: " + at);
                    }
                }
                expect(strip > 0 || F == 0 || !s.empty, "strip 0 holds column 0");
                if (strip > 0) {
                    // the row above the strip: present up to extend_band_top_hi, absent beyond
                    const int hi = extend_band_top_hi(strip, w);
                    expect(present_direct(strip * 512 - 1, hi, w) && !present_direct(strip * 512 - 1, hi + 1, w) && hi == extend_band_hi(strip * 512 - 1, w), "the row above: " + at);
                    // the diagonal input of the strip's first column comes from inside that row's window
                    if (!s.empty && s.col_first > 0) expect(present_direct(strip * 512 - 1, s.col_first - 1, w), "the column before the window is present above: " + at);
                }
                ++checked;
            }
    }
    expect(checked > 40000 && empties > 20 && unreached_seen > 1000, "the enumeration reaches empty windows and unreached read ends");

    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("extend band rules ok\n");
    return 0;
}
