// The pointer layout of banded extension alignments (versalignlib_amd/csrc/extend_band_align_plan.h) against a direct enumeration:
// every present interior cell of every strip maps inside its pair-of-pairs' region and inside its own strip's blocks, no two
// (cell, pair, word) share bits, the block counts hold at step counts = 0, 1 and 7 (mod 8), empty strips hold no block, and the
// totals are the sums of the strips' blocks -- for shapes of one to four strips and w from 0 to the unbanded limit.  A wave whose
// reference is shorter than the engine's writes a prefix of each region.  Built with -fsanitize=address,undefined and run as its
// own program.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "extend_band_align_plan.h"

using namespace valign;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            printf("FAILED %s: ", #cond);     \
            printf(__VA_ARGS__);              \
            printf("\n");                     \
            if (++failures > 20) exit(1);     \
        }                                     \
    } while (0)

// the steps of a strip by enumeration: lane l (rows [512 s + 8 l, + 8)) sweeps column j at step j + l
static void strip_steps(int strip, int F, int w, int &first, int &last, bool &any) {
    any = false;
    first = last = 0;
    for (int l = 0; l < 64; ++l) {
        const int row = strip * 512 + 8 * l;
        for (int j = 0; j < F; ++j) {
            if (!(8 * (row / 8) - w <= j && j <= 8 * (row / 8) + 7 + w)) continue;
            const int t = j + l;
            if (!any || t < first) first = t;
            if (!any || t > last) last = t;
            any = true;
        }
    }
}

static void check_shape(int R, int F, int band_width, bool affine, bool cells) {
    const int w = extend_band_half(band_width, R, F);
    const int strips = (R + 511) / 512, W = affine ? 16 : 8;
    CHECK(extend_band_align_strips(R) == strips && extend_band_align_lane_dwords(affine) == W, "R %d", R);
    long long blocks = 0;
    std::vector<long long> base(strips + 1);
    for (int s = 0; s < strips; ++s) {
        int first, last;
        bool any;
        strip_steps(s, F, w, first, last, any);
        const ExtendBandStrip win = extend_band_strip(s, F, w);
        CHECK(win.empty == !any, "R %d F %d w %d strip %d", R, F, w, s);
        const int nb = extend_band_align_strip_blocks(s, F, w);
        if (!any) {
            CHECK(nb == 0, "an empty strip holds %d blocks (R %d F %d w %d strip %d)", nb, R, F, w, s);
        } else {
            // the sweep runs the steps [t_begin, t_end): t_begin the 64-column block of the first column, t_end past the last
            // lane's last column whichever lane holds it
            CHECK(win.t_begin % 64 == 0 && win.t_begin <= first && last < win.t_end, "R %d F %d w %d strip %d", R, F, w, s);
            CHECK(nb == (win.t_end - win.t_begin + 7) / 8 && (long long)nb * 8 >= win.t_end - win.t_begin && (long long)(nb - 1) * 8 < win.t_end - win.t_begin,
                  "R %d F %d w %d strip %d: %d blocks for %d steps", R, F, w, s, nb, win.t_end - win.t_begin);
        }
        base[s] = blocks * 64 * W;
        CHECK(extend_band_align_blocks_before(s, F, w) == blocks && extend_band_align_strip_base(s, F, w, affine) == base[s], "R %d F %d w %d strip %d", R, F, w, s);
        blocks += nb;
    }
    base[strips] = blocks * 64 * W;
    const long long total = extend_band_align_pp_dwords(R, F, w, affine);
    CHECK(total == base[strips] && extend_band_align_blocks_before(strips, F, w) == blocks, "R %d F %d w %d: %lld dwords", R, F, w, total);
    if (!cells) return;
    // every present interior cell, both pairs, both words: in bounds, inside its strip, and no two share bits
    std::vector<unsigned> used((size_t)total, 0u);
    for (int i = 0; i < R; ++i) {
        const int s = i / 512;
        for (int j = 0; j < F; ++j) {
            if (!extend_band_present(i, j, w)) continue;
            for (int half = 0; half < 2; ++half) {
                for (int gap = 0; gap < (affine ? 2 : 1); ++gap) {
                    const ExtendBandAlignSlot slot = extend_band_align_slot(i, j, half, gap != 0, F, w, affine);
                    CHECK(slot.dword >= base[s] && slot.dword < base[s + 1], "cell (%d, %d) of R %d F %d w %d: dword %lld outside strip %d [%lld, %lld)", i, j, R, F, w,
                          slot.dword, s, base[s], base[s + 1]);
                    CHECK(slot.shift >= 16 * half && slot.shift + 2 <= 16 * half + 16 && slot.shift % 2 == 0, "cell (%d, %d): shift %d", i, j, slot.shift);
                    if (slot.dword < 0 || slot.dword >= total) continue;
                    const unsigned bits = 3u << slot.shift;
                    CHECK((used[(size_t)slot.dword] & bits) == 0u, "cell (%d, %d) half %d word %d of R %d F %d w %d shares its bits", i, j, half, gap, R, F, w);
                    used[(size_t)slot.dword] |= bits;
                    // the walk's own form: word() from the strip's base
                    const int l = (i % 512) / 8, t = j + l;
                    const long long same = base[s] + extend_band_align_word((t - extend_band_strip(s, F, w).t_begin) / 8, l, i % 8 + (gap ? 8 : 0), affine);
                    CHECK(same == slot.dword && slot.shift == extend_band_align_shift(t, half), "cell (%d, %d)", i, j);
                }
            }
        }
    }
}

int main() {
    // block counts at step counts = 0, 1, 7 (mod 8): one strip, the unbanded limit, t_end - t_begin = F + 63
    for (int F : {1, 2, 8, 9, 57, 64, 65, 66, 72, 73})
        for (int affine = 0; affine < 2; ++affine) {
            const int steps = F + 63, nb = extend_band_align_strip_blocks(0, F, 10000);
            CHECK(nb == (steps + 7) / 8, "F %d: %d blocks", F, nb);
            check_shape(40, F, 20000, affine != 0, true);
        }
    CHECK((64 + 63) % 8 == 7 && (65 + 63) % 8 == 0 && (66 + 63) % 8 == 1, "the residues");
    // one to four strips, w from 0 to the limit, both gap models; the cells of every shape
    const int shapes[][2] = {{33, 70}, {512, 64}, {513, 63}, {513, 129}, {520, 600}, {1030, 1100}, {1024, 300}, {1537, 1400}, {2048, 1900}, {1600, 40}};
    for (const auto &sh : shapes)
        for (int bw : {0, 1, 2, 3, 16, 17, 40, 127, 128, 130, 512, 1000, 2 * 2048, 100000})
            for (int affine = 0; affine < 2; ++affine) check_shape(sh[0], sh[1], bw, affine != 0, true);
    // a shorter reference of the same engine: a prefix of every strip's blocks, the same t_begin
    for (int w : {0, 20, 200, 5000})
        for (int s = 0; s < 4; ++s)
            for (int F2 : {0, 1, 63, 64, 500, 1099}) {
                const ExtendBandStrip big = extend_band_strip(s, 1100, w), small = extend_band_strip(s, F2, w);
                if (s > 0 && small.empty) continue;          // (the wave returns before it writes)
                CHECK(small.t_begin == big.t_begin && small.t_end <= big.t_end, "w %d strip %d F %d", w, s, F2);
                CHECK((small.t_end - small.t_begin + 7) / 8 <= extend_band_align_strip_blocks(s, 1100, w), "w %d strip %d F %d", w, s, F2);
            }
    // long reads: totals only
    for (int bw : {1, 200, 512, 1000, 40000})
        for (int affine = 0; affine < 2; ++affine) check_shape(10000, 10000, bw, affine != 0, false);
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("extend band align plan ok\n");
    return 0;
}
