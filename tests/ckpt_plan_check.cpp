// ckpt_plan_check.cpp -- the plan of the checkpointed traceback (versalignlib_amd/csrc/ckpt_plan.h) and its route
// (cell_rules.h: AlignRoute::StripCkpt) on the CPU.  Plain g++, no HIP (tests/test_ckpt_plan.py builds and runs it;
// tools/sanitize.sh runs it under UBSan).
#include <stdio.h>

#include <string>

#include "cell_rules.h"
#include "ckpt_plan.h"

using namespace valign;

namespace {

int failures = 0;
void expect(bool ok, const std::string &what) {
    if (ok) return;
    if (++failures <= 20) fprintf(stderr, "FAIL: %s\n", what.c_str());
}

unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
unsigned rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}
template <typename T, size_t N>
T pick(const T (&v)[N]) {
    return v[rnd() % N];
}

// ---- 1. bytes per pair-of-pairs: the formula of the issue, restated here with its own arithmetic ----
void check_bytes() {
    const int Rs[] = {1, 511, 512, 513, 1024, 1025, 2049, 3000, 4100, 10000, 16383, 32000};
    const int Fs[] = {1, 57, 58, 64, 300, 700, 3500, 9000, 10000, 16384};
    const int Ks[] = {8, 12, 16};
    for (int R : Rs)
        for (int F : Fs)
            for (int K : Ks)
                for (int affine = 0; affine < 2; ++affine) {
                    const CkptPlan p = ckpt_plan(R, F, K, affine != 0);
                    const std::string at = std::to_string(R) + " x " + std::to_string(F) + ", K " + std::to_string(K) + (affine ? ", affine" : "");
                    const long long S = (R + 64 * K - 1) / (64 * K);
                    const long long P = (long long)((F + 70) / 8) * 64 * K * 4 * (affine ? 2 : 1);
                    const long long row_dwords = ((F + 71) / 64 + 2) * 64;
                    const long long sets = affine ? 2 : 1;
                    expect(p.strips == S && p.rows == 64 * K && p.pad_total == S * 64 * K - R, "strips: " + at);
                    expect(p.pad_total >= 0 && p.pad_total < p.rows, "padding stays inside strip 0: " + at);
                    expect((long long)p.region_bytes == P, "one pointer region: " + at);
                    expect((long long)p.row_bytes == (S - 1) * sets * row_dwords * 4, "S - 1 row sets: " + at);
                    expect(p.state_bytes == 2 * (size_t)kWalkStateBytes, "walk state of two pairs: " + at);
                    expect((long long)p.bytes_per_pp == P + (S - 1) * sets * row_dwords * 4 + 2 * kWalkStateBytes, "bytes per pair-of-pairs: " + at);
                    expect((long long)p.full_bytes == S * P, "the full-pointer plan: " + at);
                    // a boundary row covers the 64-column loads and stores of a sweep of F + 63 steps
                    expect(p.row_dwords % 64 == 0 && p.row_dwords >= F + 135 - 64 && p.blocks8 * 8 >= F + 63, "row and block sizes: " + at);
                    // every cell of the strip has its pointer inside the one region: step t = j + lane < blocks8 * 8
                    expect((long long)p.blocks8 * 8 > (long long)(F - 1) + 63, "the region holds every step: " + at);
                }
    // the figures the header and the README quote: 10 kbp x 10 kbp, 16 rows per lane
    const CkptPlan lin = ckpt_plan(10000, 10000, 16, false), aff = ckpt_plan(10000, 10000, 16, true);
    expect(lin.strips == 10 && lin.full_bytes == 51527680ull && lin.region_bytes == 5152768ull && lin.row_bytes == 9ull * 10176 * 4, "10 kbp figures (linear)");
    expect(aff.full_bytes == 2 * lin.full_bytes && aff.row_bytes == 2 * lin.row_bytes, "10 kbp figures (affine)");
    expect(5 * lin.bytes_per_pp <= lin.full_bytes && 5 * aff.bytes_per_pp <= aff.full_bytes, "factor 5 at 10 kbp, K = 16");
    for (int K : Ks) expect(5 * ckpt_plan(10000, 10000, K, false).bytes_per_pp <= ckpt_plan(10000, 10000, K, false).full_bytes, "factor 5 at 10 kbp, every K");
}

// ---- 2. chunks under a cap; 3. the rounds ----
void check_chunks_and_rounds() {
    for (int it = 0; it < 200000; ++it) {
        const size_t bytes_per_pp = (size_t)pick({48u, 1000u, 40000u, 1u << 20, 5519176u, 51527680u, 103055360u});
        const size_t cap = (size_t)pick({1ull << 20, 4ull << 20, 256ull << 20, 24ull << 30, 128ull << 30}) + rnd() % 4096;
        const long long n = pick({1ll, 2ll, 3ll, 9ll, 64ll, 4095ll, 4096ll, 16384ll, 1000001ll});
        const long long chunk = strip_chunk_pairs(cap, bytes_per_pp, n);
        expect(chunk >= 2 && chunk % 2 == 0, "whole waves");
        expect(chunk <= (n + 1) / 2 * 2, "no more than the batch");
        // a chunk exceeds the cap only where one wave alone does (the smallest launch there is)
        expect((size_t)(chunk / 2) * bytes_per_pp <= cap || chunk == 2, "chunk under the cap");
        // ... and is the largest such: one more wave would pass the cap or the batch
        expect(chunk == (n + 1) / 2 * 2 || (size_t)(chunk / 2 + 1) * bytes_per_pp > cap, "chunk fills the cap");
        long long covered = 0;
        for (long long begin = 0; begin < n; begin += chunk) covered += std::min(chunk, n - begin);
        expect(covered == n, "chunks cover the batch");
    }
    for (int S = 1; S <= 40; ++S) {
        const std::vector<int> r = ckpt_rounds(S);
        bool ok = (int)r.size() == S;
        for (int k = 0; ok && k < S; ++k) ok = r[k] == S - 1 - k;
        expect(ok, "rounds run S - 1 .. 0 at S = " + std::to_string(S));
    }
    // the strip of a row: padding above row 0, "before the read" in strip 0, the last row in the last strip
    for (int R : {1, 1023, 1024, 1025, 3000, 10000})
        for (int K : {8, 12, 16}) {
            const CkptPlan p = ckpt_plan(R, 100, K, false);
            expect(ckpt_strip_of_row(-1, p.pad_total, p.rows) == 0 && ckpt_strip_of_row(0, p.pad_total, p.rows) == 0, "first rows in strip 0");
            expect(ckpt_strip_of_row(R - 1, p.pad_total, p.rows) == p.strips - 1, "last row in the last strip");
            for (int i = 1; i < R; ++i) {
                const int s = ckpt_strip_of_row(i, p.pad_total, p.rows), before = ckpt_strip_of_row(i - 1, p.pad_total, p.rows);
                if (s != before && !(s == before + 1 && i == s * p.rows - p.pad_total)) expect(false, "strips change at their first row");
            }
        }
}

// ---- 4. the route: StripCkpt exactly where the key is on and the call would take the plain strips with the default
// tie-breaks (traceback_policy = 1 keeps the full-pointer strips); every other route, and every refusal, as without the key ----
bool route_of(const RuleInputs &in, int alg, const RouteFacts &f, AlignRoute &route, std::string &what) {
    try {
        route = align_route(in, alg, f);
        return true;
    } catch (const std::runtime_error &e) {
        what = e.what();
        return false;
    }
}

void check_route() {
    long long ckpt_seen = 0, strip_kept = 0, others = 0, refused = 0;
    for (int it = 0; it < 400000; ++it) {
        RuleInputs in;
        const int m = pick({1, 2, 5, 60, 300, 5000}), mm = -pick({0, 1, 4, 200}), g = -pick({0, 1, 3, 80, 8000}), g2 = -pick({1, 3, 80});
        in.sc.match = m;
        in.sc.mismatch = mm;
        in.sc.gap_read = in.sc.open_read = in.sc.ext_read = g;
        in.sc.gap_ref = in.sc.open_ref = in.sc.ext_ref = g2;
        in.sc.affine = rnd() % 2;
        if (in.sc.affine) {
            in.sc.open_read = g - pick({0, 5, 700});
            in.sc.open_ref = g2 - pick({0, 5, 700});
        }
        in.R = pick({1, 64, 150, 1024, 1025, 3000, 10000});
        in.F = pick({5, 128, 500, 8092, 10000});
        in.sse_policy = rnd() % 4 == 0;
        in.no_tag = rnd() % 8 == 0;
        const int alg = rnd() % 2;
        RouteFacts off;
        off.banded = rnd() % 4 == 0;
        off.wide_align = rnd() % 8 == 0;
        off.read_strips = in.R > 1024 || rnd() % 4 == 0;
        off.fused_off = rnd() % 4 == 0;
        off.small_call = rnd() % 2;
        off.fused_rows = 256;
        RouteFacts on = off;
        on.checkpoints = true;
        AlignRoute r_off = AlignRoute::Register, r_on = AlignRoute::Register;
        std::string w_off, w_on;
        const bool ok_off = route_of(in, alg, off, r_off, w_off), ok_on = route_of(in, alg, on, r_on, w_on);
        expect(ok_off == ok_on && w_off == w_on, "the key refuses nothing and excuses nothing");
        if (!ok_off) {
            ++refused;
            continue;
        }
        expect(r_off != AlignRoute::StripCkpt, "no checkpoints without the key");
        const bool want = r_off == AlignRoute::Strip && !in.sse_policy;
        expect((r_on == AlignRoute::StripCkpt) == want, "StripCkpt exactly where the plain default-policy strips would run");
        if (!want) expect(r_on == r_off, "every other route as without the key");
        expect(strip_chunks(r_on, on) == strip_chunks(r_off, off), "the host path sizes its chunks alike");
        if (want) ++ckpt_seen;
        else if (r_off == AlignRoute::Strip) ++strip_kept;
        else ++others;
    }
    expect(ckpt_seen > 1000 && strip_kept > 100 && others > 1000 && refused > 100, "every case reached");
    expect(std::string(ran_fill_name(AlignRoute::StripCkpt)) == "strip_ckpt" && std::string(ran_fill_name(AlignRoute::Strip)) == "strip" &&
               std::string(ran_fill_name(AlignRoute::StripWideBand)) == "strip_wide_band",
           "path names");
    expect(!RouteFacts{}.checkpoints, "the key is off by default");
}

}  // namespace

int main() {
    check_bytes();
    check_chunks_and_rounds();
    check_route();
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("ckpt plan ok\n");
    return 0;
}
