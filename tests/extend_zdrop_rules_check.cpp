// The extend_zdrop key's rule (versalignlib_amd/csrc/extend_zdrop.h) on the CPU:
//   extend_zdrop_choice / extend_zdrop_align_choice over Z x band x extend_band x extend_band_align x extend_wide x score_width x
//                 policy x mode x shape x scoring: Z = 0 is extend_choice / extend_align_choice; Z > 0 every branch, with its text;
//   extend_zdrop_step against a direct restatement in 64 bits on random row-maxima sequences;
//   extend_zdrop_combine: associative, and exclusive scan + predicate per row == the serial loop (the kernel's epilogue, 64 lanes
//                 of 8 rows, seeded with a carried running best);
//   extend_zdrop_strip_skipped / extend_zdrop_unreached / the key's range.
#include "extend_zdrop.h"

#include <stdio.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

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

bool same(const PlacedChoice &a, const PlacedChoice &b) { return a.route == b.route && std::string(a.reason) == b.reason && a.key_bits == b.key_bits; }
bool same(const ExtendAlignChoice &a, const ExtendAlignChoice &b) {
    return a.route == b.route && std::string(a.reason) == b.reason && a.blocks8 == b.blocks8 && a.wave_ptr_bytes == b.wave_ptr_bytes && a.band_half == b.band_half;
}
bool begins(const char *text, const char *with) { return !strncmp(text, with, strlen(with)); }

struct Row {
    int i, m, c;
    bool counts;            // in the read and with a present candidate
};

// the definition, restated: 64-bit arithmetic, no shared code
long long direct_drop(const std::vector<Row> &rows, long long &M, long long &Mi, long long &Mj, long long Z, long long p_ref, long long p_read, long long none) {
    for (const Row &r : rows) {
        if (!r.counts) continue;
        if (r.m > M) {
            M = r.m;
            Mi = r.i;
            Mj = r.c;
            continue;
        }
        const long long di = r.i - Mi, dj = r.c - Mj;
        const long long pen = di > dj ? (di - dj) * p_ref : (dj - di) * p_read;
        if (M - r.m - pen > Z) return r.i;
    }
    return none;
}

void check_choices() {
    const int shapes[][2] = {{33, 70}, {150, 500}, {520, 600}, {1024, 1300}, {1025, 1300}, {10000, 10000}};
    const Scoring scorings[] = {lin(2, -1, -3, -3), lin(2, -1, -2, -4), aff(2, -1, -5, -1, -5, -1), aff(2, -1, -6, -2, -4, -1),
                                lin(970, -1, -3, -3), lin(2, -1, -320, -320), lin(2, -1, -30000, -30000), lin(30000, -1, -3, -3)};
    long long cells = 0, wide = 0, wide_16 = 0, wide_range = 0, mode = 0, policy_n = 0, band_on = 0, band_off = 0, band_refused = 0;
    long long aln_band = 0, aln_band_refused = 0, aln_text = 0, aln_first = 0;
    for (const auto &shape : shapes)
        for (const Scoring &sc : scorings)
            for (int width : {0, 16, 32})
                for (int band : {0, 1, 40, 100000})
                    for (bool policy : {false, true})
                        for (int alg : {kAlgSW, kAlgNW})
                            for (int bits = 0; bits < 16; ++bits)
                                for (int Z : {0, 1, 400, 1 << 29, 1 << 30}) {
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
                                    f.extend_band_align = bits & 8;
                                    const PlacedChoice plain = extend_choice(in, alg, f, 16, 10);
                                    const ExtendAlignChoice plain_aln = extend_align_choice(in, alg, f, 16, 10);
                                    const PlacedChoice c = extend_zdrop_choice(in, alg, f, 16, 10, Z);
                                    const ExtendAlignChoice a = extend_zdrop_align_choice(in, alg, f, 16, 10, Z);
                                    ++cells;
                                    if (Z == 0) {
                                        expect(same(c, plain) && same(a, plain_aln), "Z = 0: exactly the choices without the key");
                                        continue;
                                    }
                                    // ---- scores ----
                                    if (alg != kAlgSW) {
                                        expect(c.route == PlacedRoute::Refused && std::string(c.reason) == kNwText, "scores: the mode bit first, with its text");
                                        ++mode;
                                    } else if (policy) {
                                        expect(c.route == PlacedRoute::Refused && std::string(c.reason) == kPolicyText, "scores: traceback_policy = 1, with its text");
                                        ++policy_n;
                                    } else if (band > 0) {
                                        expect(same(c, plain), "scores under a band: extend_choice's answer");
                                        if (!f.extend_band) {
                                            expect(c.route == PlacedRoute::Refused && std::string(c.reason) == kBandText, "the band's refusal without extend_band");
                                            ++band_off;
                                        } else if (c.route == kPlacedRouteBand)
                                            ++band_on;
                                        else {
                                            expect(begins(c.reason, "extend_band:"), "Band's own refusals");
                                            ++band_refused;
                                        }
                                    } else if (width == 16) {
                                        expect(c.route == PlacedRoute::Refused && std::string(c.reason) == kExtendZdropNoInt16 && begins(c.reason, "extend_zdrop:"), "score_width = 16");
                                        ++wide_16;
                                    } else if (!extend_int32_ok(in)) {
                                        expect(c.route == PlacedRoute::Refused && std::string(c.reason) == kExtendZdropRange && begins(c.reason, "extend_zdrop:"), "the int32 range");
                                        ++wide_range;
                                    } else {
                                        expect(c.route == PlacedRoute::Wide && std::string(c.reason).empty(), "Wide whatever extend_wide, the read length and score_width 0 / 32 say");
                                        ++wide;
                                    }
                                    // ---- alignments ----
                                    if (alg != kAlgSW || policy) {
                                        expect(a.route == PlacedRoute::Refused && std::string(a.reason) == (alg != kAlgSW ? kNwText : kPolicyText), "alignments: the mode bit and the policy first");
                                        ++aln_first;
                                    } else if (band > 0 && f.extend_band && f.extend_band_align) {
                                        expect(same(a, plain_aln), "alignments on the banded route: as without the key");
                                        if (a.route == kPlacedRouteBand) ++aln_band;
                                        else {
                                            expect(begins(a.reason, "extend_band:"), "the banded route's refusals");
                                            ++aln_band_refused;
                                        }
                                    } else {
                                        expect(a.route == PlacedRoute::Refused && std::string(a.reason) == kExtendZdropAlign && begins(a.reason, "extend_zdrop:") &&
                                                   strstr(a.reason, "a band of 2 * max(read_length, ref_length) is the unbanded alignment"),
                                               "alignments off the banded route: one text");
                                        ++aln_text;
                                    }
                                }
    expect(wide > 0 && wide_16 > 0 && wide_range > 0 && mode > 0 && policy_n > 0 && band_on > 0 && band_off > 0 && band_refused > 0, "every branch of the scores' choice was visited");
    expect(aln_band > 0 && aln_band_refused > 0 && aln_text > 0 && aln_first > 0, "every branch of the alignments' choice was visited");
    printf("choices: %lld cells, %lld Wide, %lld Band, %lld banded alignments\n", cells, wide, band_on, aln_band);
}

void check_rule() {
    std::mt19937 rng(20240531);
    auto pick = [&](int lo, int hi) { return (int)(lo + (long long)(rng() % (unsigned)(hi - lo + 1))); };
    constexpr int kLanes = 64, kRows = 8;
    long long dropped = 0, kept = 0, scans = 0;
    for (int round = 0; round < 4000; ++round) {
        const int Z = round % 7 == 0 ? (1 << 29) : (round % 5 == 0 ? pick(1, 1 << 30) : pick(1, 200));
        const int p_ref = pick(0, 40), p_read = pick(0, 40);
        const int row0 = 512 * pick(0, 3), Rp = row0 + pick(0, 512);
        const bool big = round % 11 == 0;                   // values at the edge of the cell range
        std::vector<Row> rows;
        int walk = pick(-50, 50), col = pick(-1, 600);
        for (int r = 0; r < kLanes * kRows; ++r) {
            walk += pick(-12, 10);
            col = std::max(-1, col + pick(-2, 3));
            const int m = big ? pick(-(1 << 28), 1 << 28) : walk;
            rows.push_back(Row{row0 + r, m, col, row0 + r < Rp && pick(0, 19) != 0});
        }
        ExtendZdropBest seed = extend_zdrop_anchor();
        if (row0 > 0 && pick(0, 3)) seed = ExtendZdropBest{big ? pick(1, 1 << 28) : pick(1, 300), pick(0, row0 - 1), pick(-1, 32000)};
        expect(extend_zdrop_from_record(seed.m, seed.i + 1, seed.j + 1).i == seed.i && extend_zdrop_from_record(seed.m, seed.i + 1, seed.j + 1).j == seed.j, "the record round trip");
        // the direct restatement
        long long M = seed.m, Mi = seed.i, Mj = seed.j;
        const long long T_direct = direct_drop(rows, M, Mi, Mj, Z, p_ref, p_read, kExtendZdropNone);
        // the serial loop on the step function
        ExtendZdropBest best = seed;
        int T_serial = kExtendZdropNone;
        for (const Row &r : rows)
            if (r.counts && extend_zdrop_step(best, r.i, r.m, r.c, Z, p_ref, p_read)) {
                T_serial = r.i;
                break;
            }
        expect(T_serial == T_direct && best.m == M && best.i == Mi && best.j == Mj, "the step function against the direct restatement");
        if (Z >= (1 << 29)) expect(T_serial == kExtendZdropNone, "Z >= 2^29 never drops");
        (T_serial == kExtendZdropNone ? kept : dropped) += 1;
        // the epilogue: per lane arg-max, exclusive scan with the combine, seeded; per lane walk; the minimum
        ExtendZdropBest lane_best[kLanes], run[kLanes];
        for (int l = 0; l < kLanes; ++l) {
            lane_best[l] = extend_zdrop_no_row();
            for (int q = 0; q < kRows; ++q) {
                const Row &r = rows[l * kRows + q];
                if (r.counts) lane_best[l] = extend_zdrop_combine(lane_best[l], ExtendZdropBest{r.m, r.i, r.c});
            }
            run[l] = lane_best[l];
        }
        for (int d = 1; d < kLanes; d <<= 1) {          // the doubling steps of the wave's scan
            ExtendZdropBest next[kLanes];
            for (int l = 0; l < kLanes; ++l) next[l] = l >= d ? extend_zdrop_combine(run[l - d], run[l]) : run[l];
            for (int l = 0; l < kLanes; ++l) run[l] = next[l];
        }
        int T_scan = kExtendZdropNone;
        ExtendZdropBest at_T = extend_zdrop_combine(seed, run[kLanes - 1]);
        for (int l = 0; l < kLanes; ++l) {
            ExtendZdropBest b = l == 0 ? seed : extend_zdrop_combine(seed, run[l - 1]);
            int T = kExtendZdropNone;
            for (int q = 0; q < kRows; ++q) {
                const Row &r = rows[l * kRows + q];
                if (T == kExtendZdropNone && r.counts && extend_zdrop_step(b, r.i, r.m, r.c, Z, p_ref, p_read)) T = r.i;
            }
            if (T < T_scan) {
                T_scan = T;
                at_T = b;
            }
        }
        expect(T_scan == T_serial && at_T.m == best.m && at_T.i == best.i && at_T.j == best.j, "scan + predicate == the serial loop");
        ++scans;
        // associativity on this round's values
        for (int k = 0; k + 2 < kLanes; k += 7) {
            const ExtendZdropBest &x = lane_best[k], &y = lane_best[k + 1], &z = lane_best[k + 2];
            const ExtendZdropBest left = extend_zdrop_combine(extend_zdrop_combine(x, y), z), right = extend_zdrop_combine(x, extend_zdrop_combine(y, z));
            expect(left.m == right.m && left.i == right.i && left.j == right.j, "the combine is associative");
        }
    }
    // ties: the earlier row keeps the best
    const ExtendZdropBest a{5, 3, 9}, b{5, 4, 1}, c{6, 5, 2};
    expect(extend_zdrop_combine(a, b).i == 3 && extend_zdrop_combine(a, c).i == 5 && extend_zdrop_combine(c, a).i == 5, "a later row wins only with a strictly larger value");
    expect(extend_zdrop_combine(a, extend_zdrop_no_row()).i == 3, "no row changes nothing");
    expect(dropped > 500 && kept > 500, "sequences that drop and sequences that do not: " + std::to_string(dropped) + " / " + std::to_string(kept));
    // the step at the edges of its int32 range: M = 2^28, m = -2^28, the largest penalty
    {
        ExtendZdropBest best{1 << 28, 0, -1};
        expect(extend_zdrop_step(best, 1, -(1 << 28), -1, (1 << 29) - 1, 0, 0), "2^29 > 2^29 - 1 drops");
        expect(!extend_zdrop_step(best, 1, -(1 << 28), -1, 1 << 29, 0, 0), "2^29 > 2^29 does not");
        expect(!extend_zdrop_step(best, 32767, -(1 << 28), -1, 1, 32768, 32768), "the largest penalty stays inside int32");
    }
    printf("rule: %lld scans, %lld dropped\n", scans, dropped);
}

void check_skip_and_key() {
    const int none = kExtendZdropNone;
    expect(!extend_zdrop_strip_skipped(0, 0, 0) && !extend_zdrop_strip_skipped(0, 5, 7), "strip 0 always runs");
    expect(extend_zdrop_strip_skipped(1, 100, 511) && !extend_zdrop_strip_skipped(1, 100, 512) && !extend_zdrop_strip_skipped(1, 512, 100), "T == row0 is not yet known: the strip runs");
    expect(!extend_zdrop_strip_skipped(1, 100, none) && !extend_zdrop_strip_skipped(1, none, none) && !extend_zdrop_strip_skipped(5, none, 3), "an undropped pair keeps the wave");
    expect(extend_zdrop_strip_skipped(2, 0, 1023) && !extend_zdrop_strip_skipped(2, 0, 1024) && extend_zdrop_strip_skipped(40, 20000, 20479), "later strips");
    expect(extend_zdrop_unreached(3, 4) && !extend_zdrop_unreached(4, 4) && !extend_zdrop_unreached(none, 32767), "T < Rp: the read end is unreached");
    expect(extend_zdrop_key_ok(0) && extend_zdrop_key_ok(1) && extend_zdrop_key_ok(1ll << 30) && !extend_zdrop_key_ok(-1) && !extend_zdrop_key_ok((1ll << 30) + 1), "the key's range");
    expect(std::string(kExtendZdropKeyRange) == "extend_zdrop must be in [0, 2^30]", "the key's text");
    expect(!extend_zdrop_on(0) && extend_zdrop_on(1) && extend_zdrop_price(-7) == 7 && extend_zdrop_price(0) == 0, "on / price");
}

}  // namespace

int main() {
    check_choices();
    check_rule();
    check_skip_and_key();
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("extend zdrop rules ok\n");
    return 0;
}
