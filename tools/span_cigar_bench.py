"""What spanned CIGARs cost against full alignments: align_span_device, align_cigar_device, score_span_device and
score_placed_device in one process on short reads against references of growing length -- 150 x 500 (1,048,576 pairs), 150 x
2,000 (262,144 pairs), 150 x 8,000 (65,536 pairs) --, SW linear 2 / -1 / -3 and SW affine open -5, extend -1.

  python -m tools.span_cigar_bench [--pairs-500 1048576] [--pairs-2000 262144] [--pairs-8000 65536] [--reps 7] [--out FILE]

Inputs are resident on the device; every call is timed with events around it on one stream after two warm-up calls; the median
and the minimum of --reps launches are printed.  Beside the four calls, two calls of a child-shaped engine -- shape (R,
span_ref_length) on a batch of that shape -- are timed: score_placed_device (the reverse sweep of a spanned score call, so that
rest = span - placed - reverse sweep is what the reversal and the records kernel take) and align_cigar_device (the fill, the
walk and the encoder of the window).

PREDICTION, printed with every leg BEFORE align_span_device is timed:  placed(R, F) + align_cigar(R, Fr) + rest.  After the run
the measured time and the miss in per cent follow, whichever way it falls, and the ratio to align_cigar_device of the full shape
in the same process.  --out appends the whole report to a file (profiles/).
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
    reads, refs = synth.make_pairs(min(n, block), R, F, seed=seed, sub_rate=0.1, indel_rate=0.01)
    reps = (n + len(reads) - 1) // len(reads)
    return np.tile(reads, (reps, 1))[:n].copy(), np.tile(refs, (reps, 1))[:n].copy()


def leg(name, R, F, n, scoring, reps, lines, stride=64):
    reads, refs = _batch(n, R, F, 7, 4096)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    cells = float(n) * R * F
    results = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def report(call, med, best, ran, swept=cells):
        results.append({"leg": name, "call": call, "ms_median": round(med, 3), "ms_min": round(best, 3), "tcups": round(swept / med / 1e9, 3), "ran": ran})
        say("%-22s %-36s %10.3f ms (min %10.3f)  %7.3f TCUPS  %s" % (name, call, med, best, swept / med / 1e9, ran))

    eng = hipkernel.Engine(R, F, scoring)
    placed = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    t_placed, best = _timed(lambda: eng.score_placed_device(0, d_reads, d_refs, out=placed), reps)
    report("score_placed_device", t_placed, best, eng.describe(0, n)["ran_placed"])
    spans = torch.empty((n, 5), dtype=torch.int32, device="cuda")
    t_span, best = _timed(lambda: eng.score_span_device(0, d_reads, d_refs, out=spans), reps)
    d = eng.describe(0, n)
    Fr = d["span_ref_length"]
    window = float(n) * R * Fr
    report("score_span_device", t_span, best, "%s Fr=%d" % (d["ran_span"], Fr), cells + window)
    recs = torch.empty((n, 6), dtype=torch.int32, device="cuda")
    ops = torch.empty((n, stride), dtype=torch.int32, device="cuda")
    t_cigar, best = _timed(lambda: eng.align_cigar_device(0, d_reads, d_refs, ops_stride=stride, out=(recs, ops)), reps)
    d = eng.describe(0, n)
    report("align_cigar_device", t_cigar, best, "%s ptr=%d B/pair rows=%.0f MB" % (d["ran_align_fill"], d["align_ptr_bytes_per_pair"], d["cigar_rows_scratch_bytes"] / 1e6))
    full_ptr = d["align_ptr_bytes_per_pair"]
    eng.close()
    # the child's shape on a batch of that shape (what is swept and walked, not what is found, sets the time)
    child = hipkernel.Engine(R, Fr, scoring)
    child_refs = d_refs[:, :Fr].contiguous()
    child_placed = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    t_rev, best = _timed(lambda: child.score_placed_device(0, d_reads, child_refs, out=child_placed), reps)
    report("child score_placed_device (R x Fr)", t_rev, best, child.describe(0, n)["ran_placed"], window)
    child_recs = torch.empty((n, 6), dtype=torch.int32, device="cuda")
    child_ops = torch.empty((n, stride), dtype=torch.int32, device="cuda")
    t_child, best = _timed(lambda: child.align_cigar_device(0, d_reads, child_refs, ops_stride=stride, out=(child_recs, child_ops)), reps)
    d = child.describe(0, n)
    report("child align_cigar_device (R x Fr)", t_child, best, "%s ptr=%d B/pair" % (d["ran_align_fill"], d["align_ptr_bytes_per_pair"]), window)
    child_ptr = d["align_ptr_bytes_per_pair"]
    child.close()
    del child_refs, child_placed, child_recs, child_ops
    rest = t_span - t_placed - t_rev
    predicted = t_placed + t_child + rest
    say("%-22s PREDICTION placed(R, F) + align_cigar(R, Fr) + rest = %.3f + %.3f + %.3f = %.3f ms (align_cigar_device of the full shape: %.3f ms)" %
        (name, t_placed, t_child, rest, predicted, t_cigar))
    eng = hipkernel.Engine(R, F, scoring)
    s_recs = torch.empty((n, 6), dtype=torch.int32, device="cuda")
    s_ops = torch.empty((n, stride), dtype=torch.int32, device="cuda")
    t_aspan, best = _timed(lambda: eng.align_span_device(0, d_reads, d_refs, ops_stride=stride, out=(s_recs, s_ops)), reps)
    d = eng.describe(0, n)
    report("align_span_device", t_aspan, best, "%s scratch=%.0f MB" % (d["ran_span_cigar"], d["span_cigar_scratch_bytes"] / 1e6), cells + window)
    eng.close()
    say("%-22s measured %.3f ms: miss %+.1f %% of the prediction; align_span / align_cigar = %.2f, align_span / score_span = %.2f" %
        (name, t_aspan, 100.0 * (t_aspan - predicted) / predicted, t_aspan / t_cigar, t_aspan / t_span))
    per_pair = 3 * (R + Fr) + 20
    say("%-22s per pair: window scratch %d B + pointers %d B, against rows %d B + pointers %d B of the full alignment" %
        (name, per_pair, child_ptr, 2 * (R + F), full_ptr))
    same = bool((s_recs[:, [4, 1, 3]] == placed).all()) and bool((s_recs[:, :4] == spans[:, 1:]).all())
    hit = spans[:, 0] > 0
    agree = int(((s_recs[:, 0] == recs[:, 0]) & (s_recs[:, 2] == recs[:, 2]) & (s_recs[:, 5] == recs[:, 5]))[hit].sum())
    say("%-22s score and ends == placed, coordinates == spans: %s; begin and n_ops == the forward walk's on %d of %d pairs with a score" %
        (name, same, agree, int(hit.sum())))
    results.append({"leg": name, "consistent": same, "span_ref_length": Fr, "predicted_ms": round(predicted, 3), "rest_ms": round(rest, 3),
                    "measured_ms": round(t_aspan, 3), "miss_percent": round(100.0 * (t_aspan - predicted) / predicted, 1),
                    "span_over_cigar": round(t_aspan / t_cigar, 3), "window_bytes_per_pair": per_pair + child_ptr,
                    "full_bytes_per_pair": 2 * (R + F) + full_ptr, "same_as_forward_walk": agree, "pairs_with_score": int(hit.sum())})
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs-500", type=int, default=1 << 20)
    ap.add_argument("--pairs-2000", type=int, default=1 << 18)
    ap.add_argument("--pairs-8000", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    linear = hipkernel.Scoring.make(2, -1, -3, -3)
    affine = hipkernel.Scoring.make(2, -1, -3, -3, -5, -1, -5, -1)
    out, lines = [], ["span_cigar_bench: " + " ".join(sys.argv[1:]), "device: " + torch.cuda.get_device_name(0)]
    for F, n in ((500, args.pairs_500), (2000, args.pairs_2000), (8000, args.pairs_8000)):
        if n <= 0:
            continue
        for name, sc in (("SW linear", linear), ("SW affine", affine)):
            out += leg("150x%d %s" % (F, name), 150, F, n, sc, args.reps, lines)
    summary = json.dumps({"tool": "span_cigar_bench", "results": out})
    print(summary)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n" + summary + "\n")


if __name__ == "__main__":
    main()
