// extend_align_choice under the extend_band_align key (versalignlib_amd/csrc/cell_rules.h) on the CPU, over
// key x band x extend_band x extend_wide x score_width x policy x mode x shape x scoring:
//   key off ..... the answer -- route, text, blocks, bytes -- is the one the rule gave before the key existed, restated below
//                 (before_the_key) from extend_choice and the texts it had then;
//   key on ...... without a band or without extend_band: the same; with both: Band with the plan's blocks and bytes
//                 (extend_band_align_plan.h) wherever banded extension scores run, and their refusals, with their texts, where
//                 they do not.
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

const char *const kNwText = "extension scores are defined for opt & 0xF == 0 only (the NW variant's free reference start is another matrix)";
const char *const kPolicyText = "extension scores are not built for traceback_policy = 1 (SSE/AVX tie-breaks)";
const char *const kBandText = "extension scores are not built for band_width > 0";
const char *const kNoBandText = "extension alignments: not built under a band (extend_band = 1 runs the extension scores of this call on the banded int32 sweep, which keeps no back pointers)";
const char *const kNoWideText = "extension alignments: not built for the int32 / row-strip route of extend_wide = 1 (the extension scores of this call run there)";

// the rule as it stood before the key, from extend_choice alone
ExtendAlignChoice before_the_key(const RuleInputs &in, int alg, PlacedFacts f, int G, int K) {
    ExtendAlignChoice c;
    if (f.band_width > 0 && f.extend_band) {
        f.extend_band = false;
        f.extend_wide = false;
        const PlacedChoice plain = extend_choice(in, alg, f, G, K);
        c.reason = std::string(plain.reason) == kBandText ? kNoBandText : plain.reason;
        return c;
    }
    const PlacedChoice scores = extend_choice(in, alg, f, G, K);
    if (f.extend_wide && scores.route != PlacedRoute::Rows) {
        PlacedFacts narrow = f;
        narrow.extend_wide = false;
        const PlacedChoice plain = extend_choice(in, alg, narrow, G, K);
        c.reason = (scores.route == PlacedRoute::Wide || std::string(scores.reason) != plain.reason) ? kNoWideText : plain.reason;
        return c;
    }
    if (scores.route != PlacedRoute::Rows) {
        c.reason = scores.reason;
        return c;
    }
    c.route = PlacedRoute::Rows;
    c.blocks8 = (in.F + G - 1 + 7) / 8;
    c.wave_ptr_bytes = (long long)c.blocks8 * 64 * K * 4 * (in.sc.affine ? 2 : 1);
    return c;
}

bool same(const ExtendAlignChoice &a, const ExtendAlignChoice &b) {
    return a.route == b.route && std::string(a.reason) == b.reason && a.blocks8 == b.blocks8 && a.wave_ptr_bytes == b.wave_ptr_bytes;
}

}  // namespace

int main() {
    const int shapes[][2] = {{33, 70}, {150, 500}, {520, 600}, {1024, 1300}, {1025, 1300}, {10000, 10000}};
    const Scoring scorings[] = {lin(2, -1, -3, -3), lin(2, -1, -2, -4), aff(2, -1, -5, -1, -5, -1), aff(2, -1, -6, -2, -4, -1),
                                lin(970, -1, -3, -3), lin(2, -1, -320, -320), lin(2, -1, -30000, -30000), lin(30000, -1, -3, -3)};
    long long cells = 0, bands = 0, band_16 = 0, band_range = 0, band_mode = 0, band_policy = 0;
    for (const auto &shape : shapes)
        for (const Scoring &sc : scorings)
            for (int width : {0, 16, 32})
                for (int band : {0, 1, 40, 1000, 100000})
                    for (bool policy : {false, true})
                        for (int alg : {kAlgSW, kAlgNW})
                            for (int bits = 0; bits < 16; ++bits) {
                                RuleInputs in;
                                in.sc = sc;
                                in.R = shape[0];
                                in.F = shape[1];
                                in.sse_policy = policy;
                                in.no_f16 = true;
                                PlacedFacts f{};
                                f.band_width = band;
                                f.score_width = width;
                                f.forced = bits & 1;
                                f.long_plan = shape[0] > 2048;
                                f.extend_wide = bits & 2;
                                f.extend_band = bits & 4;
                                f.band_placed = f.chain_usable = bits & 8;
                                expect(!f.extend_band_align, "the key is off by default");
                                const ExtendAlignChoice before = before_the_key(in, alg, f, 16, 10);
                                expect(same(extend_align_choice(in, alg, f, 16, 10), before), "key off: the answer of before the key");
                                expect(before.route != kPlacedRouteBand && before.band_half == 0, "key off: never Band");
                                f.extend_band_align = true;
                                const ExtendAlignChoice on = extend_align_choice(in, alg, f, 16, 10);
                                ++cells;
                                if (band == 0 || !f.extend_band) {
                                    expect(same(on, before), "key on without a band or without extend_band: not read");
                                    continue;
                                }
                                const PlacedChoice scores = extend_choice(in, alg, f, 16, 10);
                                if (alg != kAlgSW) {
                                    expect(on.route == PlacedRoute::Refused && std::string(on.reason) == kNwText, "the mode bit, with its text");
                                    ++band_mode;
                                } else if (policy) {
                                    expect(on.route == PlacedRoute::Refused && std::string(on.reason) == kPolicyText, "traceback_policy = 1, with its text");
                                    ++band_policy;
                                } else if (width == 16) {
                                    expect(on.route == PlacedRoute::Refused && std::string(on.reason) == kExtendBandNoInt16 && !strncmp(on.reason, "extend_band:", 12), "score_width = 16");
                                    ++band_16;
                                } else if (!extend_band_int32_ok(in)) {
                                    expect(on.route == PlacedRoute::Refused && std::string(on.reason) == kExtendBandRange && !strncmp(on.reason, "extend_band:", 12), "the range");
                                    ++band_range;
                                } else {
                                    const int w = extend_band_half(band, in.R, in.F);
                                    expect(scores.route == kPlacedRouteBand && on.route == kPlacedRouteBand && std::string(on.reason).empty(), "Band wherever the scores run banded");
                                    expect(on.band_half == w && on.wave_ptr_bytes == 4 * extend_band_align_pp_dwords(in.R, in.F, w, sc.affine) && on.wave_ptr_bytes > 0,
                                           "the plan's pointer bytes");
                                    expect(on.blocks8 == extend_band_align_blocks_before(extend_band_align_strips(in.R), in.F, w) &&
                                               on.wave_ptr_bytes == (long long)on.blocks8 * 64 * 4 * (sc.affine ? 16 : 8),
                                           "the plan's blocks");
                                    ++bands;
                                }
                            }
    expect(bands > 0 && band_16 > 0 && band_range > 0 && band_mode > 0 && band_policy > 0, "every branch was visited");
    // the figure of the issue's arithmetic: 10 kbp x 10 kbp under band_width 512, per PAIR
    {
        const int w = extend_band_half(512, 10000, 10000);
        const long long lin_pair = 4 * extend_band_align_pp_dwords(10000, 10000, w, false) / 2, aff_pair = 4 * extend_band_align_pp_dwords(10000, 10000, w, true) / 2;
        expect(aff_pair == 2 * lin_pair && lin_pair > 2500000 && lin_pair < 3200000, "about 2.9 / 5.9 MB per pair: " + std::to_string(lin_pair));
        printf("10 kbp x 10 kbp, band_width 512: %lld / %lld pointer bytes per pair (linear / affine)\n", lin_pair, aff_pair);
    }
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("extend band align rules ok (%lld cells, %lld Band)\n", cells, bands);
    return 0;
}
