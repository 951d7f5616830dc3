"""What extension scores cost: score_extend_device beside score_placed_device (on a scoring that takes the placed sweep's rows
track: match 14, beyond the lane key at 150 rows) and align_cigar_device with opt = 1 -- the call a caller had to make for a
gap-priced border -- in one process on the bench batch (1,048,576 pairs of 150 x 500), linear gaps 14 / -7 / -21 and affine gaps
open -35, extend -7.

  python -m tools.extend_bench [--pairs 1048576] [--reps 7] [--out FILE]

Inputs are resident on the device; every call is timed with events around it on one stream after two warm-up calls; the median
and the minimum of --reps launches are printed.

PREDICTION, printed BEFORE the extension call is timed: the rows-track placed time x the ratio of VALU instructions per step pair
at 16 x 10 (tools/isa_histogram.py: 214 / 189 for the symmetric linear form, 298 / 273 for the symmetric affine form), and the miss
of the measurement against it.  --out appends the whole report to a file (profiles/).
"""
import argparse
import json
import statistics
import sys

import numpy as np
import torch

from versalignlib_amd import hipkernel, synth

# VALU instructions of the two-step trip at 16 x 10: (score_extend_kernel, score_placed_kernel's rows track), by gap form
VALU_PER_STEP_PAIR = {"linear": (214, 189), "affine": (298, 273)}


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


def leg(name, form, R, F, n, scoring, reps, lines):
    reads, refs = synth.make_pairs(min(n, 4096), R, F, seed=7, sub_rate=0.1, indel_rate=0.01)
    tiles = (n + len(reads) - 1) // len(reads)
    reads, refs = np.tile(reads, (tiles, 1))[:n].copy(), np.tile(refs, (tiles, 1))[:n].copy()
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    cells = float(n) * R * F
    results = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def report(call, med, best, ran):
        results.append({"leg": name, "call": call, "ms_median": round(med, 3), "ms_min": round(best, 3), "tcups": round(cells / med / 1e9, 3), "ran": ran})
        say("%-18s %-30s %10.3f ms (min %10.3f)  %7.3f TCUPS  %s" % (name, call, med, best, cells / med / 1e9, ran))

    eng = hipkernel.Engine(R, F, scoring)
    placed = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    t_placed, best = _timed(lambda: eng.score_placed_device(0, d_reads, d_refs, out=placed), reps)
    report("score_placed_device", t_placed, best, eng.describe(0, n)["ran_placed"])
    ext_valu, placed_valu = VALU_PER_STEP_PAIR[form]
    predicted = t_placed * ext_valu / placed_valu
    say("%-18s predicted score_extend_device = placed x %d / %d = %.3f ms" % (name, ext_valu, placed_valu, predicted))
    ext = torch.empty((n, 5), dtype=torch.int32, device="cuda")
    t_ext, best = _timed(lambda: eng.score_extend_device(0, d_reads, d_refs, out=ext), reps)
    report("score_extend_device", t_ext, best, eng.describe(0, n)["ran_extend"])
    say("%-18s measured %.3f ms: miss %+.1f %%; extend / placed = %.3f" % (name, t_ext, 100.0 * (t_ext - predicted) / predicted, t_ext / t_placed))
    consistent = bool((ext[:, 0] <= placed[:, 0]).all())
    recs = torch.empty((n, 6), dtype=torch.int32, device="cuda")
    ops = torch.empty((n, 64), dtype=torch.int32, device="cuda")
    t_cigar, best = _timed(lambda: eng.align_cigar_device(1, d_reads, d_refs, ops_stride=64, out=(recs, ops)), reps)
    report("align_cigar_device opt = 1", t_cigar, best, eng.describe(1, n)["ran_align_fill"])
    say("%-18s extend / cigar(opt = 1) = %.3f; extension score <= placed score on every pair: %s; pairs that extend: %d of %d" %
        (name, t_ext / t_cigar, consistent, int((ext[:, 0] > 0).sum()), n))
    eng.close()
    results.append({"leg": name, "predicted_ms": round(predicted, 3), "miss_percent": round(100.0 * (t_ext - predicted) / predicted, 2), "consistent": consistent})
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    linear = hipkernel.Scoring.make(14, -7, -21, -21)
    affine = hipkernel.Scoring.make(14, -7, -21, -21, -35, -7, -35, -7)
    out, lines = [], ["extend_bench: " + " ".join(sys.argv[1:]), "device: " + torch.cuda.get_device_name(0)]
    out += leg("150x500 linear", "linear", 150, 500, args.pairs, linear, args.reps, lines)
    out += leg("150x500 affine", "affine", 150, 500, args.pairs, affine, args.reps, lines)
    summary = json.dumps({"tool": "extend_bench", "results": out})
    print(summary)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n" + summary + "\n")


if __name__ == "__main__":
    main()
