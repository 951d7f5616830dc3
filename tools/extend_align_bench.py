"""What extension alignments cost: align_extend_device at end_bonus = -1 (the best cell) and INT32_MAX (always the read end) beside
score_extend_device, align_cigar_device with opt = 0 and align_cigar_device under the debug switch no_tag -- the equality-test
Smith-Waterman fill, the comparable one -- in one process on the bench batch (1,048,576 pairs of 150 x 500), linear gaps 2 / -1 /
-2 / -4 and affine gaps open -6 / -4, extend -2 / -1 (the general forms: the two directions differ).

  python -m tools.extend_align_bench [--pairs 1048576] [--reps 7] [--out FILE]

Inputs are resident on the device; every call is timed with events around it on one stream after two warm-up calls; the median
and the minimum of --reps launches are printed.

PREDICTION, printed BEFORE the extension alignments are timed: the no_tag call's time x the ratio of VALU instructions per step pair
of the two fills at 16 x 10 (tools/isa_histogram.py, the hot loops of align_extend_fill_kernel and of align_fill_kernel /
align_fill_affine_kernel) -- the walk and the encoder are inside the no_tag call's time already, and are taken as equal -- and the
miss of each measurement against it.  Also printed: pointer-scratch bytes per pair and the size of libHIPKernel.so.  --out appends
the whole report to a file (profiles/).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

from versalignlib_amd import build, hipkernel, synth

# VALU instructions of the two-step trip at 16 x 10: (align_extend_fill_kernel, the equality-test Smith-Waterman fill), by gap model
VALU_PER_STEP_PAIR = {"linear": (359, 333), "affine": (561, 440)}
INT32_MAX = 2 ** 31 - 1


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


def _engine(R, F, scoring, **debug):
    """an engine created under VALIGN_HIP_DEBUG = debug (read when the engine is created), the variable restored behind it"""
    before = os.environ.get("VALIGN_HIP_DEBUG")
    if debug:
        os.environ["VALIGN_HIP_DEBUG"] = ",".join("%s=%d" % kv for kv in debug.items())
    try:
        return hipkernel.Engine(R, F, scoring)
    finally:
        if before is None:
            os.environ.pop("VALIGN_HIP_DEBUG", None)
        else:
            os.environ["VALIGN_HIP_DEBUG"] = before


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
        say("%-18s %-38s %10.3f ms (min %10.3f)  %7.3f TCUPS  %s" % (name, call, med, best, cells / med / 1e9, ran))

    recs = torch.empty((n, 6), dtype=torch.int32, device="cuda")
    ops = torch.empty((n, 64), dtype=torch.int32, device="cuda")
    ext = torch.empty((n, 5), dtype=torch.int32, device="cuda")
    eng = _engine(R, F, scoring)
    t_scores, best = _timed(lambda: eng.score_extend_device(0, d_reads, d_refs, out=ext), reps)
    report("score_extend_device", t_scores, best, eng.describe(0, n)["ran_extend"])
    scores = ext.clone()
    t_cigar, best = _timed(lambda: eng.align_cigar_device(0, d_reads, d_refs, ops_stride=64, out=(recs, ops)), reps)
    report("align_cigar_device opt = 0", t_cigar, best, eng.describe(0, n)["ran_align_fill"])
    plain = _engine(R, F, scoring, no_tag=1)
    t_plain, best = _timed(lambda: plain.align_cigar_device(0, d_reads, d_refs, ops_stride=64, out=(recs, ops)), reps)
    d = plain.describe(0, n)
    report("align_cigar_device opt = 0, no_tag", t_plain, best, "%s, %d pointer bytes per pair" % (d["ran_align_fill"], d["align_ptr_bytes_per_pair"]))
    plain.close()
    new_valu, fill_valu = VALU_PER_STEP_PAIR[form]
    predicted = t_plain * new_valu / fill_valu
    say("%-18s predicted align_extend_device = no_tag x %d / %d = %.3f ms" % (name, new_valu, fill_valu, predicted))
    for bonus, label in ((-1, "end_bonus = -1"), (INT32_MAX, "end_bonus = INT32_MAX")):
        t_new, best = _timed(lambda: eng.align_extend_device(0, d_reads, d_refs, end_bonus=bonus, ops_stride=64, out=(recs, ops, ext)), reps)
        d = eng.describe(0, n)
        report("align_extend_device " + label, t_new, best, "%s on %s" % (d["ran_extend_align"], d["ran_extend_align_geometry"]))
        same = bool((ext == scores).all())
        say("%-18s %s: measured %.3f ms, miss %+.1f %%; / no_tag = %.3f, / cigar = %.3f, / score_extend = %.3f; extension records equal score_extend_device's: %s; "
            "non-empty alignments: %d of %d, mean ops %.2f" % (name, label, t_new, 100.0 * (t_new - predicted) / predicted, t_new / t_plain, t_new / t_cigar,
                                                               t_new / t_scores, same, int((recs[:, 5] > 0).sum()), n, float(recs[:, 5].float().mean())))
        results.append({"leg": name, "bonus": bonus, "predicted_ms": round(predicted, 3), "miss_percent": round(100.0 * (t_new - predicted) / predicted, 2),
                        "records_equal": same})
    G, K = (int(v) for v in eng.describe(0, n)["ran_extend_align_geometry"].split("x"))
    blocks = (F + G - 1 + 7) // 8
    say("%-18s pointer scratch: %d bytes per pair (%d blocks x %d lanes x %d dwords per pair-of-pairs); scratch held: %d bytes" %
        (name, G * blocks * K * 4 * (2 if form == "affine" else 1) // 2, blocks, G, K * (2 if form == "affine" else 1), eng.describe(0, n)["extend_align_scratch_bytes"]))
    eng.close()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    linear = hipkernel.Scoring.make(2, -1, -2, -4)
    affine = hipkernel.Scoring.make(2, -1, -3, -3, -6, -2, -4, -1)
    out, lines = [], ["extend_align_bench: " + " ".join(sys.argv[1:]), "device: " + torch.cuda.get_device_name(0),
                      "libHIPKernel.so: %d bytes" % os.path.getsize(build.HIP_PLUGIN)]
    print("\n".join(lines), flush=True)
    out += leg("150x500 linear", "linear", 150, 500, args.pairs, linear, args.reps, lines)
    out += leg("150x500 affine", "affine", 150, 500, args.pairs, affine, args.reps, lines)
    summary = json.dumps({"tool": "extend_align_bench", "results": out})
    print(summary)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n" + summary + "\n")


if __name__ == "__main__":
    main()
