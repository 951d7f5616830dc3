// The extend_zdrop_rows key's rule (versalignlib_amd/csrc/extend_zdrop.h) on the CPU:
//   the lane form -- G lanes of K rows: local combine, exclusive scan seeded with the anchor, replay per lane, minimum -- against the
//                 serial loop of extend_zdrop_step, on the six (G, K) of the full geometries: random row tables, Rp at every
//                 position of a lane, ties of row maxima, drops planted at a lane's first and last row, at row 0 and at row
//                 Rp - 1, no drop, Z in {1, 2^29, 2^30} (Z = 0 is the caller's: the key is not read);
//   extend_zdrop_rows_choice / extend_zdrop_rows_align_choice over the keys x score_width x band x read length x scoring: key off
//                 is extend_zdrop_choice / extend_zdrop_align_choice with the texts they have, key on every branch.
#include "extend_zdrop.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
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

bool same(const PlacedChoice &a, const PlacedChoice &b) { return a.route == b.route && std::string(a.reason) == b.reason && a.key_bits == b.key_bits; }
bool same(const ExtendAlignChoice &a, const ExtendAlignChoice &b) {
    return a.route == b.route && std::string(a.reason) == b.reason && a.blocks8 == b.blocks8 && a.wave_ptr_bytes == b.wave_ptr_bytes && a.band_half == b.band_half;
}
bool same(const ExtendZdropBest &a, const ExtendZdropBest &b) { return a.m == b.m && a.i == b.i && a.j == b.j; }
bool begins(const char *text, const char *with) { return !strncmp(text, with, strlen(with)); }

struct Table {
    std::vector<int> m, c;          // G * K row entries; rows at and beyond Rp hold what a pad row may hold: anything
    int Rp;
};

// the serial rule: rows 0 .. Rp - 1 in order -> T (Rp where none drops) and the running best as it stands at T
int serial(const Table &t, int Z, int p_ref, int p_read, ExtendZdropBest &best) {
    best = extend_zdrop_anchor();
    for (int i = 0; i < t.Rp; ++i)
        if (extend_zdrop_step(best, i, t.m[i], t.c[i], Z, p_ref, p_read)) return i;
    return t.Rp;
}

// the lane form, as the kernel's epilogue runs it -> T and the record's running best
int lanes(const Table &t, int G, int K, int Z, int p_ref, int p_read, ExtendZdropBest &best) {
    std::vector<ExtendZdropBest> run(G);
    for (int l = 0; l < G; ++l) run[l] = extend_zdrop_lane_best(&t.m[l * K], &t.c[l * K], K, l * K, t.Rp);           // 1. the local combine
    for (int d = 1; d < G; d <<= 1) {                                                                                   // 2. the doubling steps of the scan ...
        std::vector<ExtendZdropBest> next(run);
        for (int l = d; l < G; ++l) next[l] = extend_zdrop_combine(run[l - d], run[l]);
        run = next;
    }
    std::vector<ExtendZdropLane> mine(G);
    int T = kExtendZdropNone;
    for (int l = 0; l < G; ++l) {
        const ExtendZdropBest prefix = l == 0 ? extend_zdrop_anchor() : extend_zdrop_combine(extend_zdrop_anchor(), run[l - 1]);      // ... shifted by a lane, seeded
        mine[l] = extend_zdrop_replay_lane(&t.m[l * K], &t.c[l * K], K, l * K, t.Rp, kExtendZdropNone, prefix, Z, p_ref, p_read);  // 3. the replay
        T = std::min(T, mine[l].T);                                                                                     // 4. the minimum
    }
    T = std::min(T, t.Rp);
    if (t.Rp == 0) {
        best = extend_zdrop_anchor();
        return 0;
    }
    const int src = extend_zdrop_record_lane(T, t.Rp, K);
    best = mine[src].best;
    // the replay of lane T / K stopped at T is the same record, whatever that lane answered by itself
    const ExtendZdropBest prefix = src == 0 ? extend_zdrop_anchor() : extend_zdrop_combine(extend_zdrop_anchor(), run[src - 1]);
    const ExtendZdropLane stopped = extend_zdrop_replay_lane(&t.m[src * K], &t.c[src * K], K, src * K, t.Rp, T, prefix, Z, p_ref, p_read);
    expect(stopped.T == kExtendZdropNone && same(stopped.best, best), "the replay stopped at T: no drop before it, the same running best");
    return T;
}

long long compared = 0, dropped = 0, kept = 0;
void compare(const Table &t, int G, int K, int Z, int p_ref, int p_read, const std::string &what, int want_T = -1) {
    ExtendZdropBest a, b;
    const int Ts = serial(t, Z, p_ref, p_read, a), Tl = lanes(t, G, K, Z, p_ref, p_read, b);
    expect(Ts == Tl && same(a, b), what + ": lane form == serial loop (" + std::to_string(G) + " x " + std::to_string(K) + ", Rp " + std::to_string(t.Rp) + ", T " +
                                       std::to_string(Ts) + " / " + std::to_string(Tl) + ")");
    if (want_T >= 0) expect(Ts == want_T, what + ": the planted drop row " + std::to_string(want_T) + ", not " + std::to_string(Ts));
    ++compared;
    (Ts < t.Rp ? dropped : kept) += 1;
}

// a homology down the diagonal -- row i's maximum 2 (i + 1) at column i -- that ends at row `stop`: from there on the maxima stay at
// column stop - 1 and lose `fall` per row, so with prices 0 the first row more than Z below the best drops
Table homology(int G, int K, int Rp, int stop, int fall) {
    Table t{std::vector<int>(G * K), std::vector<int>(G * K), Rp};
    for (int i = 0; i < G * K; ++i) {
        t.m[i] = i < stop ? 2 * (i + 1) : 2 * stop - fall * (i - stop + 1);
        t.c[i] = i < stop ? i : stop - 1;
    }
    return t;
}

void check_lane_form(int G, int K) {
    std::mt19937 rng(977u * G + K);
    auto pick = [&](int lo, int hi) { return (int)(lo + (long long)(rng() % (unsigned)(hi - lo + 1))); };
    const int rows = G * K;
    // random tables: walks of int16 values, a few at the edges of int16, Rp anywhere
    for (int round = 0; round < 1500; ++round) {
        const int Z = round % 7 == 0 ? (1 << 29) : (round % 13 == 0 ? (1 << 30) : (round % 5 == 0 ? 1 : pick(1, 200)));
        const int p_ref = pick(0, 40), p_read = pick(0, 40);
        Table t{std::vector<int>(rows), std::vector<int>(rows), pick(0, rows)};
        const bool edge = round % 11 == 0;
        int walk = pick(-50, 50), col = pick(-1, 300);
        for (int i = 0; i < rows; ++i) {
            walk = std::max(-32000, std::min(32000, walk + pick(-12, 11)));
            col = std::max(-1, col + pick(-2, 3));
            t.m[i] = edge ? pick(-32768, 32767) : walk;
            t.c[i] = col;
        }
        ExtendZdropBest best;
        const int T = serial(t, Z, p_ref, p_read, best);
        if (Z >= (1 << 29)) expect(T == t.Rp, "Z >= 2^29 never drops");
        compare(t, G, K, Z, p_ref, p_read, "random table");
    }
    // Rp at every position of a lane (and of its neighbours), with and without a drop above it
    for (int lane : {0, 1, G / 2, G - 1})
        for (int q = 0; q <= K; ++q) {
            const int Rp = std::min(rows, lane * K + q);
            compare(homology(G, K, Rp, Rp, 3), G, K, 5, 0, 0, "Rp inside a lane, no drop", Rp);
            if (Rp >= 4) compare(homology(G, K, Rp, Rp / 2, 3), G, K, 5, 0, 0, "Rp inside a lane, a drop above it", Rp / 2 + 1);
        }
    // drops at a lane's first and last row, at row 0 and at row Rp - 1
    for (int lane : {1, G / 2, G - 1}) {
        for (int T : {lane * K, lane * K + K - 1}) {
            // Z = 5, fall 3: row stop loses 3, row stop + 1 loses 6 > 5 -- the drop row is stop + 1
            compare(homology(G, K, rows, T - 1, 3), G, K, 5, 0, 0, "a drop at a lane's edge", T);
            compare(homology(G, K, T + 1, T - 1, 3), G, K, 5, 0, 0, "a drop at row Rp - 1", T);
            // the running best in lane 0, the drop far below it
            Table far = homology(G, K, rows, 2, 0);
            for (int i = T; i < rows; ++i) far.m[i] = -100;
            compare(far, G, K, 50, 0, 0, "the running best in lane 0", T);
        }
    }
    {
        Table t = homology(G, K, rows, 0, 3);         // nothing scores: row 0 is 3 below the anchor's 0
        compare(t, G, K, 2, 0, 0, "a drop at row 0", 0);
        compare(t, G, K, 1, 0, 0, "a drop at row 0, Z = 1", 0);
        Table one = t;
        one.Rp = 1;
        compare(one, G, K, 2, 0, 0, "a drop at row 0 = Rp - 1", 0);
        compare(homology(G, K, rows, rows, 3), G, K, 1, 0, 0, "no drop", rows);
        compare(homology(G, K, rows, 3, 3), G, K, 1 << 29, 0, 0, "no drop under 2^29", rows);
        compare(homology(G, K, rows, 3, 3), G, K, 1 << 30, 0, 0, "no drop under 2^30", rows);
        compare(homology(G, K, 0, 0, 3), G, K, 1, 0, 0, "Rp = 0", 0);
    }
    // ties of row maxima: a later row with the same maximum must not move the best -- in the same lane and across lanes
    {
        Table t{std::vector<int>(rows, 7), std::vector<int>(rows), rows};
        for (int i = 0; i < rows; ++i) t.c[i] = rows - i;
        ExtendZdropBest best;
        expect(lanes(t, G, K, 1 << 29, 1, 1, best) == rows && same(best, ExtendZdropBest{7, 0, rows}), "ties: the first row keeps the best");
        compare(t, G, K, 3, 1, 1, "ties under a small Z");
        t.m[K] = 9;                                     // lane 1's first row moves it, lane 1's later 9s and lane 2's do not
        t.m[K + 1] = 9;
        t.m[2 * K] = 9;
        expect(lanes(t, G, K, 1 << 29, 1, 1, best) == rows && same(best, ExtendZdropBest{9, K, rows - K}), "ties across lanes: the earlier row keeps the best");
        compare(t, G, K, 1, 0, 0, "ties across lanes under Z = 1");
    }
    // the arithmetic at the edge of its range on this route: M = 32767, m = -32768, the largest penalty
    {
        ExtendZdropBest best{32767, 0, -1};
        expect(extend_zdrop_step(best, 1, -32768, -1, 65534, 0, 0) && !extend_zdrop_step(best, 1, -32768, -1, 65535, 0, 0), "M - m reaches 65535");
        expect(!extend_zdrop_step(best, 32767, -32768, -1, 1, 32768, 32768), "the largest penalty stays inside int32");
    }
}

void check_choices() {
    const int shapes[][2] = {{33, 70}, {150, 500}, {520, 600}, {1024, 1300}, {1025, 1300}, {1500, 1600}, {10000, 10000}};
    const Scoring scorings[] = {lin(2, -1, -3, -3), lin(2, -1, -2, -4), aff(2, -1, -5, -1, -5, -1), aff(2, -1, -6, -2, -4, -1),
                                lin(970, -1, -3, -3), lin(2, -1, -320, -320), lin(2, -1, -30000, -30000), lin(30000, -1, -3, -3)};
    long long cells = 0, rows = 0, rows_16 = 0, wide = 0, refused = 0, aln_rows = 0, aln_text = 0, aln_band = 0, aln_first = 0, off = 0;
    for (const auto &shape : shapes)
        for (const Scoring &sc : scorings)
            for (int width : {0, 16, 32})
                for (int band : {0, 1, 40, 100000})
                    for (bool policy : {false, true})
                        for (int alg : {kAlgSW, kAlgNW})
                            for (int bits = 0; bits < 16; ++bits)
                                for (int Z : {0, 1, 400, 1 << 29, 1 << 30})
                                    for (bool key : {false, true}) {
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
                                        const PlacedChoice plain = extend_choice(in, alg, f, 16, 10), today = extend_zdrop_choice(in, alg, f, 16, 10, Z);
                                        const ExtendAlignChoice plain_aln = extend_align_choice(in, alg, f, 16, 10), today_aln = extend_zdrop_align_choice(in, alg, f, 16, 10, Z);
                                        const PlacedChoice c = extend_zdrop_rows_choice(in, alg, f, 16, 10, Z, key);
                                        const ExtendAlignChoice a = extend_zdrop_rows_align_choice(in, alg, f, 16, 10, Z, key);
                                        ++cells;
                                        if (!key || Z == 0 || band > 0) {
                                            // the key off, Z = 0 or a band: exactly today's answers, the two older texts included
                                            expect(same(c, today) && same(a, today_aln), "key off, Z = 0 or a band: today's choices");
                                            expect(!extend_zdrop_rows_runs(c, f, Z, key) && !extend_zdrop_rows_runs(a, f, Z, key), "... and no ZDROP instance of the register sweep");
                                            if (Z == 0) expect(same(c, plain) && same(a, plain_aln), "Z = 0: the call without either key");
                                            if (!key && Z > 0 && band == 0 && alg == kAlgSW && !policy) {
                                                expect(c.route != PlacedRoute::Rows, "key off: no Z-dropped call on the register route");
                                                expect(std::string(a.reason) == kExtendZdropAlign, "key off: the alignments' older text");
                                                if (width == 16) expect(std::string(c.reason) == kExtendZdropNoInt16, "key off: score_width = 16 keeps its text");
                                                ++off;
                                            }
                                            continue;
                                        }
                                        // ---- the key on, Z > 0, no band ----
                                        if (plain.route == PlacedRoute::Rows) {
                                            expect(same(c, plain) && extend_zdrop_rows_runs(c, f, Z, key), "scores: Rows where the call without Z is Rows");
                                            ++rows;
                                            if (width == 16) ++rows_16;
                                        } else {
                                            expect(same(c, today) && !extend_zdrop_rows_runs(c, f, Z, key), "scores: today's answer everywhere else");
                                            if (c.route == PlacedRoute::Wide) ++wide;
                                            else ++refused;
                                            if (alg == kAlgSW && !policy) {
                                                expect(c.route == PlacedRoute::Wide || begins(c.reason, "extend_zdrop:"), "scores off the register route: Wide or its refusals");
                                                if (width != 16 && extend_int32_ok(in)) expect(c.route == PlacedRoute::Wide, "score_width = 32, cells outside int16, reads over 1,024 rows: Wide");
                                            }
                                        }
                                        if (alg != kAlgSW || policy) {
                                            expect(same(a, plain_aln) && a.route == PlacedRoute::Refused, "alignments: the mode bit and the policy first, with their texts");
                                            ++aln_first;
                                        } else if (plain_aln.route == PlacedRoute::Rows) {
                                            expect(same(a, plain_aln) && extend_zdrop_rows_runs(a, f, Z, key) && a.wave_ptr_bytes > 0, "alignments: Rows where the call without Z is Rows");
                                            ++aln_rows;
                                        } else {
                                            expect(a.route == PlacedRoute::Refused && std::string(a.reason) == kExtendZdropRowsAlign && begins(a.reason, "extend_zdrop:") &&
                                                       strstr(a.reason, "the int32 route of unbanded extension alignments has no Z-drop form") && !extend_zdrop_rows_runs(a, f, Z, key),
                                                   "alignments off the register route: the new text");
                                            ++aln_text;
                                        }
                                    }
    // a band with both banded keys answers as today under the key (counted apart: the loop above only proves equality)
    {
        RuleInputs in;
        in.sc = lin(2, -1, -3, -3);
        in.R = 150;
        in.F = 500;
        in.no_f16 = true;
        PlacedFacts f{};
        f.band_width = 40;
        f.extend_band = f.extend_band_align = true;
        expect(extend_zdrop_rows_align_choice(in, kAlgSW, f, 16, 10, 400, true).route == kPlacedRouteBand && extend_zdrop_rows_choice(in, kAlgSW, f, 16, 10, 400, true).route == kPlacedRouteBand,
               "the banded route answers as today");
        ++aln_band;
    }
    expect(rows > 0 && rows_16 > 0 && wide > 0 && refused > 0 && off > 0, "every branch of the scores' choice was visited");
    expect(aln_rows > 0 && aln_text > 0 && aln_band > 0 && aln_first > 0, "every branch of the alignments' choice was visited");
    expect(std::string(kExtendZdropNoInt16) == "extend_zdrop: Z-dropped extension scores run on int32 cells; score_width = 16 (int16 or refuse) is refused", "the older text, word for word");
    expect(begins(kExtendZdropAlign, "extend_zdrop: Z-dropped extension alignments run on the banded route only"), "the alignments' older text");
    expect(extend_zdrop_rows_key_ok(0) && extend_zdrop_rows_key_ok(1) && !extend_zdrop_rows_key_ok(2) && !extend_zdrop_rows_key_ok(-1), "the key takes 0 or 1");
    expect(std::string(kExtendZdropRowsKeyRange) == "extend_zdrop_rows must be 0 or 1", "the key's text");
    printf("choices: %lld cells, %lld Rows (%lld under score_width = 16), %lld Wide, %lld aligned on Rows, %lld with the new text\n", cells, rows, rows_16, wide, aln_rows, aln_text);
}

}  // namespace

int main() {
    const int geometries[][2] = {{8, 8}, {16, 10}, {32, 10}, {64, 8}, {64, 16}, {64, 32}};
    for (const auto &g : geometries) check_lane_form(g[0], g[1]);
    expect(dropped > 1000 && kept > 1000, "tables that drop and tables that do not: " + std::to_string(dropped) + " / " + std::to_string(kept));
    printf("lane form: %lld tables, %lld dropped\n", compared, dropped);
    check_choices();
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("extend zdrop rows rules ok\n");
    return 0;
}
