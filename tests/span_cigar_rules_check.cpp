// span_cigar_rules_check.cpp -- CPU check of span_cigar_choice (versalignlib_amd/csrc/cell_rules.h; plain g++, no HIP;
// tests/test_span_cigar_rules.py builds and runs it, once plain and once with -fsanitize=address,undefined): what a spanned
// CIGAR call refuses, with which text, and which routes a call that runs takes.
//   1. calls that run: the forward sweep's route is span_choice's, the child's route is align_route's for the child shape
//      (R, span_ref_length) -- register sweep, row strips, checkpointed strips, int32 strips under placed_wide;
//   2. every refusal of span_choice with span_choice's own text, unprefixed;
//   3. what align_route refuses for the child, prefixed with "spanned CIGARs: ".
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

// the child's rule inputs as the engine makes them: same scoring and switches, shape (R, span_ref_length)
RuleInputs child_of(const RuleInputs &in) {
    RuleInputs c = in;
    c.F = (int)span_ref_length(in);
    return c;
}

// the child's route facts: unbanded always; strips for reads of more than 1 024 rows
RouteFacts child_facts(const RuleInputs &child, bool checkpoints = false) {
    RouteFacts f;
    f.read_strips = child.R > 1024;
    f.checkpoints = checkpoints;
    return f;
}

SpanCigarChoice choose(const RuleInputs &in, int alg, const PlacedFacts &f, bool checkpoints = false) {
    const RuleInputs child = child_of(in);
    return span_cigar_choice(in, alg, f, child, child_facts(child, checkpoints), 16, 10);
}

}  // namespace

int main() {
    const RuleInputs plain = inputs(lin(2, -1, -3, -3), 150, 500);
    const RuleInputs affine = inputs(aff(2, -1, -5, -1, -5, -1), 150, 8000);

    // ---- 1. calls that run ----
    {
        const SpanCigarChoice c = choose(plain, kAlgSW, PlacedFacts{});
        expect(!c.refused() && c.reason.empty(), "the plain call runs: " + c.reason);
        expect(c.forward.route == PlacedRoute::Key && c.child == AlignRoute::Register, "150 x 500: key forward, register child");
        expect(child_of(plain).F == 249 && child_of(affine).F == 449, "the child shapes: 249 / 449 columns");
        const SpanCigarChoice a = choose(affine, kAlgSW, PlacedFacts{});
        expect(!a.refused() && a.child == AlignRoute::Register, "150 x 8000 affine runs on the register sweep of 150 x 449");
        expect(a.forward.route == span_choice(affine, kAlgSW, PlacedFacts{}, 16, 10).route, "the forward choice is span_choice's");
        const SpanCigarChoice no_geo = span_cigar_choice(plain, kAlgSW, PlacedFacts{}, child_of(plain), child_facts(child_of(plain)));
        expect(!no_geo.refused(), "without a geometry: not refused");
    }
    {
        const RuleInputs tall = inputs(lin(2, -1, -3, -3), 1025, 1300);
        const SpanCigarChoice s = choose(tall, kAlgSW, PlacedFacts{});
        expect(!s.refused() && s.forward.route == PlacedRoute::Strip && s.child == AlignRoute::Strip, "1 025 rows: strips, both");
        const SpanCigarChoice k = choose(tall, kAlgSW, PlacedFacts{}, true);
        expect(!k.refused() && k.child == AlignRoute::StripCkpt, "trace_checkpoints: the child walks with checkpoints");
        expect(choose(plain, kAlgSW, PlacedFacts{}, true).child == AlignRoute::Register, "... and changes nothing for a short read");
    }
    {
        // placed_wide = 1: the forward sweep on int32 cells; the child picks its own cells
        PlacedFacts wide{};
        wide.placed_wide = true;
        wide.score_width = 32;
        const SpanCigarChoice w = choose(plain, kAlgSW, wide);
        expect(!w.refused() && w.forward.route == PlacedRoute::Wide && w.child == AlignRoute::Register, "score_width 32 + placed_wide: wide forward, int16 child");
        wide.score_width = 0;
        const RuleInputs big = inputs(lin(214, -1, -3, -3), 150, 500);
        const SpanCigarChoice b = choose(big, kAlgSW, wide);
        expect(!b.refused() && b.forward.route == PlacedRoute::Wide && b.child == AlignRoute::StripWide, "cells beyond int16: wide forward, int32 strips for the child");
        expect(child_of(big).F == 500, "(its child is as wide as the pair)");
    }

    // ---- 2. span_choice's refusals, with its texts ----
    auto refused = [&](const RuleInputs &in, int alg, const PlacedFacts &f, const char *word) {
        const SpanCigarChoice c = choose(in, alg, f);
        const PlacedChoice s = span_choice(in, alg, f, 16, 10);
        expect(c.refused() && c.forward.route == PlacedRoute::Refused, std::string("refused: ") + word);
        expect(s.route == PlacedRoute::Refused && c.reason == s.reason, std::string("span_choice's own text: ") + c.reason);
        expect(c.reason.find(word) != std::string::npos, std::string("... which holds '") + word + "': " + c.reason);
        expect(c.reason.find(kSpanCigarPrefix) == std::string::npos, "... unprefixed");
    };
    refused(plain, kAlgNW, PlacedFacts{}, "Smith-Waterman only");
    RuleInputs sse = plain;
    sse.sse_policy = true;
    refused(sse, kAlgSW, PlacedFacts{}, "traceback_policy = 1");
    refused(plain, kAlgSW, PlacedFacts{0, 32, false, false}, "score_width = 32");
    expect(!choose(plain, kAlgSW, PlacedFacts{0, 16, false, false}).refused(), "score_width = 16 inside int16 runs");
    refused(inputs(lin(214, -1, -3, -3), 150, 500), kAlgSW, PlacedFacts{}, "int16");
    {
        PlacedFacts sixteen{};
        sixteen.score_width = 16;
        sixteen.placed_wide = true;
        refused(inputs(lin(214, -1, -3, -3), 150, 500), kAlgSW, sixteen, "int16");                   // 16 means int16 or refuse
    }
    const char *band_text = "spanned scores are not built for band_width > 0";
    for (bool band_placed : {false, true})
        for (bool usable : {false, true}) {
            const SpanCigarChoice c = choose(plain, kAlgSW, PlacedFacts{64, 0, false, false, band_placed, usable});
            expect(c.refused() && c.reason == band_text, "band refused: " + c.reason);
        }
    refused(plain, kAlgNW, PlacedFacts{64, 0, false, false, true, true}, "Smith-Waterman only");      // an unbanded refusal first, under a band too
    {
        PlacedFacts wide{};
        wide.placed_wide = true;
        const SpanCigarChoice c = choose(inputs(lin(8192, -1, -1, -1), 16383, 16383), kAlgSW, wide);
        expect(c.refused() && c.reason == "placed_wide: shape x scoring can leave the int32 range of the DP cells", "beyond int32: " + c.reason);
    }

    // ---- 3. the child's refusals, prefixed ----
    auto child_refused = [&](const RuleInputs &child, const RouteFacts &facts, const char *word) {
        const SpanCigarChoice c = span_cigar_choice(plain, kAlgSW, PlacedFacts{}, child, facts, 16, 10);
        std::string own;
        try {
            (void)align_route(child, kAlgSW, facts);
        } catch (const std::runtime_error &e) {
            own = e.what();
        }
        expect(!own.empty() && own.find(word) != std::string::npos, std::string("align_route refuses the child: ") + word);
        expect(c.refused() && c.forward.route == PlacedRoute::Refused && c.reason == std::string("spanned CIGARs: ") + own, "prefixed: " + c.reason);
    };
    {
        RuleInputs child = child_of(plain);
        child.sse_policy = true;
        child.sc = aff(2, -1, -5, -1, -5, -1);
        child_refused(child, RouteFacts{}, "linear gap model only");
        RouteFacts banded;
        banded.banded = true;
        child_refused(child, banded, "band_alignments needs traceback_policy = 0");
        child_refused(inputs(lin(8192, -1, -1, -1), 16383, 16383), RouteFacts{}, "int32 range");
    }

    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("span cigar rules ok\n");
    return 0;
}
