"""What spanned Smith-Waterman scores cost: score_placed_device, score_span_device and align_cigar_device in one process on the
bench batch (1,048,576 pairs of 150 x 500), on 150 x 2,000 (262,144 pairs: the clip of the reverse sweep bites) and on
10 kbp x 10 kbp (4,096 pairs: span_ref_length = ref_length, two full sweeps), SW linear 2 / -1 / -3 and SW affine open -5,
extend -1.

  python -m tools.span_bench [--short-pairs 1048576] [--wide-pairs 262144] [--long-pairs 4096] [--reps 7] [--skip-long] [--out FILE]

Inputs are resident on the device; every call is timed with events around it on one stream after two warm-up calls; the median
and the minimum of --reps launches are printed.  Beside the three calls, the reverse sweep is timed on its own -- a second engine
of shape (R, span_ref_length) running score_placed_device on a batch of that shape -- so that the two small kernels of a
spanned call (the reversal and the records) are what is left:  rest = span - placed - reverse sweep.

PREDICTION printed with every leg: placed x (1 + R x Fr / (R x F)) -- the two sweeps at the placed call's rate per cell -- and
the miss of the measured spanned call against it; `rest` over the reversal's bytes (R + F read, R + Fr written per pair) is the
rate the small kernels reached.  --out appends the whole report to a file (profiles/).
"""
import argparse
import json
import statistics
import sys

import numpy as np
import torch

from versalignlib_amd import hipkernel, synth


def _timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out)


def _batch(n, R, F, seed, block):
    reads, refs = synth.make_pairs(min(n, block), R, F, seed=seed, sub_rate=0.1, indel_rate=0.0 if R > 2000 else 0.01)
    reps = (n + len(reads) - 1) // len(reads)
    return np.tile(reads, (reps, 1))[:n].copy(), np.tile(refs, (reps, 1))[:n].copy()


def leg(name, R, F, n, scoring, reps, block, long_read, lines):
    reads, refs = _batch(n, R, F, 7, block)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    cells = float(n) * R * F
    results = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def report(call, med, best, ran, swept=cells):
        results.append({"leg": name, "call": call, "ms_median": round(med, 3), "ms_min": round(best, 3), "tcups": round(swept / med / 1e9, 3), "ran": ran})
        say("%-22s %-34s %10.3f ms (min %10.3f)  %7.3f TCUPS  %s" % (name, call, med, best, swept / med / 1e9, ran))

    eng = hipkernel.Engine(R, F, scoring)
    placed = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    t_placed, best = _timed(lambda: eng.score_placed_device(0, d_reads, d_refs, out=placed), reps)
    report("score_placed_device", t_placed, best, eng.describe(0, n)["ran_placed"])
    spans = torch.empty((n, 5), dtype=torch.int32, device="cuda")
    t_span, best = _timed(lambda: eng.score_span_device(0, d_reads, d_refs, out=spans), reps)
    d = eng.describe(0, n)
    Fr = d["span_ref_length"]
    report("score_span_device", t_span, best, "%s Fr=%d scratch=%.0f MB" % (d["ran_span"], Fr, d["span_scratch_bytes"] / 1e6), cells + float(n) * R * Fr)
    same = bool((spans[:, [0, 2, 4]] == placed).all())
    eng.close()
    # the reverse sweep alone: an engine of its shape on a batch of its shape (what it sweeps, not what it finds, sets the time)
    rev = hipkernel.Engine(R, Fr, scoring)
    rev_refs = d_refs[:, :Fr].contiguous()
    rev_out = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    t_rev, best = _timed(lambda: rev.score_placed_device(0, d_reads, rev_refs, out=rev_out), reps)
    report("reverse sweep alone (R x Fr)", t_rev, best, rev.describe(0, n)["ran_placed"], float(n) * R * Fr)
    rev.close()
    del rev_refs, rev_out
    stride = 4096 if long_read else 64
    eng = hipkernel.Engine(R, F, scoring)
    recs = torch.empty((n, 6), dtype=torch.int32, device="cuda")
    ops = torch.empty((n, stride), dtype=torch.int32, device="cuda")
    t_cigar, best = _timed(lambda: eng.align_cigar_device(0, d_reads, d_refs, ops_stride=stride, out=(recs, ops)), max(2, reps // 2) if long_read else reps)
    report("align_cigar_device", t_cigar, best, eng.describe(0, n)["ran_align_fill"])
    hit = spans[:, 0] > 0
    agree = int(((recs[:, 0] == spans[:, 1]) & (recs[:, 2] == spans[:, 3]))[hit].sum())
    same = same and bool((recs[:, 1] == spans[:, 2]).all()) and bool((recs[:, 3] == spans[:, 4]).all())
    del recs, ops
    eng.close()
    predicted = t_placed * (1.0 + Fr / float(F))
    rest = t_span - t_placed - t_rev
    moved = float(n) * (2 * R + F + Fr)
    say("%-22s predicted placed x (1 + Fr / F) = %.3f ms, measured %.3f ms: miss %+.1f %%; span / placed = %.2f, span / cigar = %.2f" %
        (name, predicted, t_span, 100.0 * (t_span - predicted) / predicted, t_span / t_placed, t_span / t_cigar))
    say("%-22s rest = span - placed - reverse sweep = %.3f ms for the reversal (%.0f MB moved: %.0f GB/s if it were all of it) and the records" %
        (name, rest, moved / 1e6, moved / max(rest, 1e-3) / 1e6))
    say("%-22s score and ends == placed and == cigar records: %s; begin == the walk's begin on %d of %d pairs with a score" % (name, same, agree, int(hit.sum())))
    results.append({"leg": name, "consistent": same, "span_ref_length": Fr, "predicted_ms": round(predicted, 3), "rest_ms": round(rest, 3),
                    "begin_equals_walk": agree, "pairs_with_score": int(hit.sum())})
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--short-pairs", type=int, default=1 << 20)
    ap.add_argument("--wide-pairs", type=int, default=1 << 18)
    ap.add_argument("--long-pairs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-long", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    linear = hipkernel.Scoring.make(2, -1, -3, -3)
    affine = hipkernel.Scoring.make(2, -1, -3, -3, -5, -1, -5, -1)
    out, lines = [], ["span_bench: " + " ".join(sys.argv[1:]), "device: " + torch.cuda.get_device_name(0)]
    for name, sc in (("SW linear", linear), ("SW affine", affine)):
        out += leg("150x500 " + name, 150, 500, args.short_pairs, sc, args.reps, 4096, False, lines)
    for name, sc in (("SW linear", linear), ("SW affine", affine)):
        out += leg("150x2000 " + name, 150, 2000, args.wide_pairs, sc, args.reps, 4096, False, lines)
    if not args.skip_long:
        for name, sc in (("SW linear", linear), ("SW affine", affine)):
            out += leg("10kx10k " + name, 10000, 10000, args.long_pairs, sc, max(3, args.reps // 2), 64, True, lines)
    summary = json.dumps({"tool": "span_bench", "results": out})
    print(summary)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n" + summary + "\n")


if __name__ == "__main__":
    main()
