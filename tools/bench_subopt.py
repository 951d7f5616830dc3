"""What suboptimal Smith-Waterman scores cost beside placed scores: score_subopt_device and score_placed_device alternating in
one process on the bench batch (1,048,576 pairs of 150 x 500, mask = 75), SW linear 2 / -1 / -3 and SW affine open -5, extend -1.

  python tools/bench_subopt.py [--pairs 1048576] [--reps 9] [--placed-only] [--tree DIR] [--out FILE]

Inputs are resident on the device; every call is timed with device events around it on one stream after two warm-up calls of
each kind; the two calls take turns, so both see the same clocks.  Median, minimum and the spread (max - min) of --reps launches
are printed, the ratio subopt / placed of the medians, and the PREDICTION made from the instruction counts before any run (below).
--placed-only times placed scores alone; with --tree it imports the package of another checkout (a parent-commit build), so that
its placed time can be taken in the same visit.  --out appends the report to a file (profiles/).

PREDICTION, made from the compiler's assembly before any run (tools/isa_histogram.py on the two-step trip of 16 x 10, key
track, weighted issue cycles per wave): linear symmetric 663 -> 738 (+11 %), affine symmetric 1,024 -> 1,084 (+6 %): the DPP
move and the maximum, and for lane G - 1 the shift, the ring address and the LDS store, which every lane of the wave pays
for, plus the scalar flush test.  The flush writes 4 bytes per pair of pairs and column -- 1.05 GB per 1,048,576 pairs of
150 x 500 -- as whole 16-byte stores, 256 contiguous bytes per group; the records kernel reads them back once, with the
references (0.52 GB): about 0.9 ms at 3 TB/s beside a 10.2 / 14.5 ms sweep, +9 % / +6 %.  Predicted ratio to placed scores:
1.20 linear, 1.12 affine.  (The rows track, taken by scorings beyond the key's range, pays an AND and a maximum per register:
770 -> 1,147 cycles on the same trip, +49 %; not on this bench.)
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

PREDICTED = {"SW linear": 1.20, "SW affine": 1.12}


def _event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--mask", type=int, default=75)
    ap.add_argument("--placed-only", action="store_true")
    ap.add_argument("--tree", default=None, help="import versalignlib_amd from this checkout instead of this one")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from versalignlib_amd import hipkernel, synth

    R, F, n = 150, 500, args.pairs
    reads, refs = synth.make_pairs(min(n, 4096), R, F, seed=7, sub_rate=0.1, indel_rate=0.01)
    tiles = (n + len(reads) - 1) // len(reads)
    d_reads = torch.from_numpy(np.tile(reads, (tiles, 1))[:n].copy()).cuda()
    d_refs = torch.from_numpy(np.tile(refs, (tiles, 1))[:n].copy()).cuda()
    lines = ["bench_subopt: " + " ".join(sys.argv[1:]), "device: " + torch.cuda.get_device_name(0), "library: " + hipkernel.plugin_path()]
    results = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for name, sc in (("SW linear", hipkernel.Scoring.make(2, -1, -3, -3)), ("SW affine", hipkernel.Scoring.make(2, -1, -3, -3, -5, -1, -5, -1))):
        eng = hipkernel.Engine(R, F, sc)
        placed = torch.empty((n, 3), dtype=torch.int32, device="cuda")
        calls = {"placed": lambda: eng.score_placed_device(0, d_reads, d_refs, out=placed)}
        if not args.placed_only:
            sub = torch.empty((n, 5), dtype=torch.int32, device="cuda")
            calls["subopt"] = lambda: eng.score_subopt_device(0, d_reads, d_refs, args.mask, out=sub)
        for _ in range(2):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                times[k].append(_event_ms(torch, fn))
        d = eng.describe(0, n)
        for k, t in times.items():
            med = statistics.median(t)
            ran = d["ran_placed"] if k == "placed" else "%s ring=%d scratch=%.0f MB" % (d["ran_subopt"], d["subopt_ring_cols"], d["subopt_scratch_bytes"] / 1e6)
            say("150x500 %-10s %-8s %9.3f ms median (min %9.3f, spread %6.3f)  %6.3f TCUPS  %s" %
                (name, k, med, min(t), max(t) - min(t), float(n) * R * F / med / 1e9, ran))
            results.append({"leg": name, "call": k, "ms_median": round(med, 3), "ms_min": round(min(t), 3), "ms_spread": round(max(t) - min(t), 3)})
        if not args.placed_only:
            ratio = statistics.median(times["subopt"]) / statistics.median(times["placed"])
            same = bool((sub[:, :3] == placed).all())
            say("150x500 %-10s subopt / placed = %.3f; predicted %.2f: %s (miss %+.1f %%); first three fields == placed records: %s; score2 > 0 on %d of %d pairs" %
                (name, ratio, PREDICTED[name], "met" if ratio <= PREDICTED[name] * 1.03 else "MISSED", 100.0 * (ratio - PREDICTED[name]) / PREDICTED[name], same,
                 int((sub[:, 3] > 0).sum()), n))
            results.append({"leg": name, "ratio": round(ratio, 3), "predicted": PREDICTED[name], "consistent": same})
        eng.close()
    summary = json.dumps({"tool": "bench_subopt", "placed_only": args.placed_only, "results": results})
    print(summary)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n" + summary + "\n")


if __name__ == "__main__":
    main()
